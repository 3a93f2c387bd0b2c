"""NumPy / SciPy restatement of include/mdvt_inspatio.h, written from the header's formulas: the six integer correlation sums of a
masked cell by direct integer correlation (scipy.signal.correlate2d on int64) and by scipy.fft in float64 plus rint, the float64
formula from the sums to the shift, the one-dimensional form of the border columns, the 4 x 4 grid of a frame, and the alignment's
flow field and warp (cv2.resize on float32: tests/metric_align_ref.py's restatement; cv2.remap in OpenCV's fixed-point path with a
replicated border)."""
import numpy as np
import scipy.fft
import scipy.signal

import metric_align_ref as mar

F = np.float32
GRID = 4
DIRECT, TRANSFORM = 1, 2


def grey(rgb):
    """OpenCV's 8-bit COLOR_RGB2GRAY."""
    c = np.asarray(rgb).astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def edges(n):
    return [g * n // GRID for g in range(GRID + 1)]


def path_of(W, H):
    """mdvt_masked_shift_path."""
    hmax, wmax = -(-H // 4), -(-W // 4)
    if W < 8 or H < 8 or hmax > 1024 or wmax > 1024:
        return 0
    return DIRECT if hmax * wmax <= 4096 else TRANSFORM


# ---- the six sums -------------------------------------------------------------------------------------------------------------------
def _terms(gI, gR, V):
    v = (np.asarray(V) != 0).astype(np.int64)
    a, b = np.asarray(gI).astype(np.int64) * v, np.asarray(gR).astype(np.int64) * v
    # (first operand at x, second at x - d): N, SF, SR, FR, FF, RR
    return [(v, v), (a, v), (v, b), (a, b), (a * a, v), (v, b * b)]


def sums_direct(gI, gR, V):
    """-> int64 [6, 2 h - 1, 2 w - 1]: N, SF, SR, FR, FF, RR at displacement (dy, dx) = index - (h - 1, w - 1)."""
    return np.stack([scipy.signal.correlate2d(x, y, mode="full") for x, y in _terms(gI, gR, V)])


def sums_fft(gI, gR, V):
    """The same by scipy.fft in float64 plus rint -> (int64 [6, 2 h - 1, 2 w - 1], the largest |x - rint(x)|)."""
    h, w = np.asarray(V).shape
    shape = (scipy.fft.next_fast_len(2 * h - 1, real=True), scipy.fft.next_fast_len(2 * w - 1, real=True))
    out, worst = [], 0.0
    spectra = {}

    def spectrum(x):
        key = x.tobytes()
        if key not in spectra:
            spectra[key] = scipy.fft.rfft2(x.astype(np.float64), shape)
        return spectra[key]

    for x, y in _terms(gI, gR, V):
        full = scipy.fft.irfft2(spectrum(x) * np.conj(spectrum(y)), shape)
        # displacement d at index d mod shape: bring -(h - 1) .. h - 1 into ascending order
        full = np.concatenate([full[shape[0] - (h - 1):], full[:h]], axis=0)
        full = np.concatenate([full[:, shape[1] - (w - 1):], full[:, :w]], axis=1)
        r = np.rint(full)
        worst = max(worst, float(np.abs(full - r).max()))
        out.append(r.astype(np.int64))
    return np.stack(out), worst


# ---- from the sums to the shift -----------------------------------------------------------------------------------------------------
def shift_of_sums(sums, centre):
    """sums float64 [6, ...] over the displacements, centre: the index of displacement 0 per axis -> the shift per axis (float64)."""
    N, SF, SR, FR, FF, RR = (np.asarray(s, np.float64) for s in sums)
    with np.errstate(all="ignore"):
        num = np.where(N == 0, 0.0, FR - (SF * SR) / N)
        fd = np.where(N == 0, 0.0, np.maximum(FF - (SF * SF) / N, 0.0))
        rd = np.where(N == 0, 0.0, np.maximum(RR - (SR * SR) / N, 0.0))
        den = np.sqrt(fd * rd)
        tol = (1000.0 * 2.0 ** -23) * den.max()
        c = np.where(den > tol, np.clip(num / den, -1.0, 1.0), 0.0)
    c = np.where(N < 0.3 * N.max(), 0.0, c)
    at = np.argwhere(c == c.max())
    return [float(-(int(at[:, k].sum()) - len(at) * centre[k])) / float(len(at)) for k in range(at.shape[1])]


def shift_2d(gI, gR, V, route=DIRECT):
    h, w = np.asarray(V).shape
    sums = sums_direct(gI, gR, V) if route == DIRECT else sums_fft(gI, gR, V)[0]
    return shift_of_sums(sums, (h - 1, w - 1))


def shift_1d(gI, gR, V):
    """The border columns' form -> dy, or None where no row has a valid pixel."""
    v = np.asarray(V) != 0
    h = v.shape[0]
    n_y = v.sum(axis=1)
    cnt = np.where(n_y > 0, n_y.astype(F), F(1e-8)).astype(F)
    r = ((np.asarray(gR).astype(np.int64) * v).sum(axis=1).astype(F) / cnt).astype(F)
    q = ((np.asarray(gI).astype(np.int64) * v).sum(axis=1).astype(F) / cnt).astype(F)
    rows = n_y > 0
    if not rows.any():
        return None
    sums = np.zeros((6, 2 * h - 1), np.float64)
    for i in range(2 * h - 1):
        dy = i - (h - 1)
        acc = [0.0] * 6
        for y in range(max(0, dy), min(h, h + dy)):
            if rows[y] and rows[y - dy]:
                a, b = float(q[y]), float(r[y - dy])
                acc = [acc[0] + 1.0, acc[1] + a, acc[2] + b, acc[3] + a * b, acc[4] + a * a, acc[5] + b * b]
        sums[:, i] = acc
    return shift_of_sums(sums, (h - 1,))[0]


def shift_grid(R, I, V, route=None):
    """One frame: R, I uint8 [H, W, 3], V [H, W] -> (shift float64 [4, 4, 2] (dy, dx), status uint8 [4, 4])."""
    H, W = np.asarray(V).shape
    route = path_of(W, H) if route is None else route
    gR, gI, v = grey(R), grey(I), np.asarray(V) != 0
    ye, xe = edges(H), edges(W)
    shift, status = np.zeros((GRID, GRID, 2), np.float64), np.zeros((GRID, GRID), np.uint8)
    for gy in range(GRID):
        for gx in range(GRID):
            sl = (slice(ye[gy], ye[gy + 1]), slice(xe[gx], xe[gx + 1]))
            pv = v[sl]
            if float(pv.sum()) / float(pv.size) < 0.2:
                continue
            if gx in (0, GRID - 1):
                dy = shift_1d(gI[sl], gR[sl], pv)
                if dy is None:
                    continue
                shift[gy, gx], status[gy, gx] = (dy, 0.0), 1
            else:
                shift[gy, gx], status[gy, gx] = shift_2d(gI[sl], gR[sl], pv, route), 1
    return shift, status


# ---- the flow field and the warp ----------------------------------------------------------------------------------------------------
def flow_maps(grid, W, H):
    """grid float32 [4, 4, 2] (dx, dy) -> (map_x, map_y) float32 [H, W]: fl32(x - flow_dx), fl32(y - flow_dy)."""
    fdx, fdy = mar.resize_linear(grid[..., 0], W, H), mar.resize_linear(grid[..., 1], W, H)
    xs, ys = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
    return (xs - fdx).astype(F), (ys - fdy).astype(F)


def remap_replicate(src, map_x, map_y):
    """cv2.remap(INTER_LINEAR, BORDER_REPLICATE) of uint8 [H, W, 3] in OpenCV's fixed-point path: coordinates rounded to 1 / 32 pixel
    (a tie to the even one), integer weights of sum 2^15, (sum + 2^14) >> 15; the four taps' coordinates clamped to the image."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape[:2]
    sx = np.rint(np.asarray(map_x, F) * F(32)).astype(np.int64)
    sy = np.rint(np.asarray(map_y, F) * F(32)).astype(np.int64)
    ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31
    acc = np.zeros(src.shape, np.int64)
    for t, wgt in enumerate(((32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32)):
        tx, ty = np.clip(ix + (t & 1), 0, W - 1), np.clip(iy + (t >> 1), 0, H - 1)
        acc += wgt[..., None] * src[ty, tx].astype(np.int64)
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def warp(frame, grid):
    H, W = frame.shape[:2]
    return remap_replicate(frame, *flow_maps(grid, W, H))


# ---- the frame preparation ------------------------------------------------------------------------------------------------------------
def prepare_eye(sbs_color, sbs_mask, eye, model_w, model_h):
    """One side-by-side frame pair [H, 2 W, 3] -> (V [H, W], render [H, W, 3], model V [mh, mw], model render [mh, mw, 3], holes):
    mdvt_inspatio_prepare_eye (the u8 resize is tests/infill_adapter_ref.py's restatement)."""
    import infill_adapter_ref as iar
    W = sbs_color.shape[1] // 2
    color, mask = sbs_color[:, eye * W:(eye + 1) * W], sbs_mask[:, eye * W:(eye + 1) * W]
    V = np.where((mask != 0).any(axis=2), 0, 255).astype(np.uint8)
    render = np.where((V == 0)[..., None], 0, color).astype(np.uint8)
    mv = iar.resize_u8(np.repeat(V[..., None], 3, axis=2), model_w, model_h)[..., 0]
    return V, render, mv, iar.resize_u8(render, model_w, model_h), int((V == 0).sum())


# ---- the compositing ------------------------------------------------------------------------------------------------------------------
def gauss_blur5(plane):
    """cv2.GaussianBlur(plane, (5, 5), 0) of a float32 plane with BORDER_REFLECT_101: the fixed table 1 4 6 4 1 / 16 per axis."""
    w = np.array([1, 4, 6, 4, 1], F) / F(16)
    H, W = plane.shape
    p = np.pad(plane.astype(F), ((0, 0), (2, 2)), mode="reflect")
    acc = sum(w[i] * p[:, i:i + W] for i in range(5))
    p = np.pad(acc.astype(F), ((2, 2), (0, 0)), mode="reflect")
    out = sum(w[i] * p[i:i + H] for i in range(5))
    return out.astype(F)


def composite_eye(aligned, sbs_color, sbs_mask, eye, orc, blend=True):
    """aligned [H, W, 3] and one side-by-side frame pair -> (pasted, blended or None) of that eye: mdvt_inspatio_composite_eye.  orc:
    the module whose mark_lower_side stands for the reference's (oracle/c_oracle.py)."""
    from scipy.ndimage import binary_dilation
    W = sbs_color.shape[1] // 2
    color, mask = sbs_color[:, eye * W:(eye + 1) * W], np.ascontiguousarray(sbs_mask[:, eye * W:(eye + 1) * W])
    hole = (mask != 0).any(axis=2)
    pasted = np.where(hole[..., None], aligned, color).astype(np.uint8)
    if not blend:
        return pasted, None
    blue = orc.mark_lower_side(mask, 30)
    marks = (blue == np.array([0, 0, 255], np.uint8)).all(axis=-1)
    grown = binary_dilation(marks, iterations=3) if marks.any() else marks
    alpha = gauss_blur5(grown.astype(F))[..., None]
    v = (alpha * aligned.astype(F)).astype(F) + ((F(1) - alpha).astype(F) * pasted.astype(F)).astype(F)
    assert v.dtype == F
    return pasted, np.clip(v, 0, 255).astype(np.uint8)


# ---- the step end to end ----------------------------------------------------------------------------------------------------------------
def _padded(a, T):
    return a if len(a) == T else np.concatenate([a, np.repeat(a[-1:], T - len(a), axis=0)], axis=0)


def deal_with_frame_chunk(first, color, mask, org, last, fps, generate, orc, blend, model_size, text_prompt):
    """One chunk on the host (tools/inspatio_world_infill.py's deal_with_frame_chunk).  generate(source, render, mask, fps, text_prompt)
    -> frames on NumPy arrays.  The grid clean-up is the package's (NumPy, held by hand-made grids in tests/test_inspatio_cpu.py).
    -> (start, pasted, blended) of the written frames."""
    import infill_adapter_ref as iar
    from metric_depth_video_toolbox_amd import inspatio_world as iw
    T, H, W = len(color), color.shape[1], color.shape[2] // 2
    mw, mh = model_size
    start, end = (0 if first else 3), (T if last else T - 3)
    Tp = iw.pad_to_valid_T(T)
    eyes = [[prepare_eye(color[k], mask[k], eye, mw, mh) for k in range(T)] for eye in (0, 1)]
    holes = [[e[4] for e in eyes[eye]] for eye in (0, 1)]
    source = _padded(np.stack([iar.resize_u8(f, mw, mh) for f in org]), Tp) if (sum(holes[0]) + sum(holes[1])) else None
    halves = []
    for eye in (0, 1):
        valid, render = np.stack([e[0] for e in eyes[eye]]), np.stack([e[1] for e in eyes[eye]])
        if not sum(holes[eye]):
            aligned = render
        else:
            frames = generate(source, _padded(np.stack([e[3] for e in eyes[eye]]), Tp), _padded(np.stack([e[2] for e in eyes[eye]]), Tp), fps, text_prompt)
            assert frames.shape == (Tp, mh, mw, 3) and frames.dtype == np.uint8
            back = np.stack([iar.resize_u8(f, W, H) for f in frames[:T]])
            both = [shift_grid(render[k], back[k], valid[k]) for k in range(T)]
            grids, has = iw.flow_grids(np.stack([b[0] for b in both]), np.stack([b[1] for b in both]), holes[eye])
            aligned = np.stack([warp(back[k], grids[k]) if has[k] else back[k] for k in range(T)])
        done = [composite_eye(aligned[k], color[k], mask[k], eye, orc, blend) for k in range(start, end)]
        halves.append(([d[0] for d in done], [d[1] if blend else d[0] for d in done]))
    if end <= start:
        empty = np.empty((0,) + color.shape[1:], np.uint8)
        return start, empty, empty
    return start, np.concatenate([np.stack(halves[0][0]), np.stack(halves[1][0])], axis=2), np.concatenate([np.stack(halves[0][1]), np.stack(halves[1][1])], axis=2)


def run_clip(color, mask, org, fps, generate, orc, blend, model_size, chunk, text_prompt):
    """The whole schedule on host arrays: color [N, H, 2W, 3], mask [M, H, 2W, 3] (M < N: black masks for the rest), org [>= N, oh, ow,
    3] -> (output frames [N, H, 2W, 3], [(first, last, buffered frames)] per call).  After a chunk six frames are kept: three pasted
    ones with their own masks and original frames, then three untouched ones."""
    n = len(color)
    full_mask = np.zeros_like(color)
    full_mask[:min(n, len(mask))] = mask[:n]
    out, calls, buf, first = [], [], [], True

    def call(last):
        c, m, o = (np.array([b[i] for b in buf]) for i in range(3))
        calls.append((first, last, len(buf)))
        return (c, m, o) + deal_with_frame_chunk(first, c, m, o, last, fps, generate, orc, blend, model_size, text_prompt)
    for t in range(n):
        buf.append((color[t], full_mask[t], org[t]))
        if len(buf) >= chunk:
            c, m, o, start, pasted, blended = call(False)
            out.extend(blended)
            T = len(buf)
            buf = [(pasted[T - 6 - start + i], m[T - 6 + i], o[T - 6 + i]) for i in range(3)] + buf[-3:]
            first = False
    out.extend(call(True)[5])
    return np.array(out), calls
