"""The expected values of the MegaSAM camera-tracking step's tests: NumPy restatements of the four entry points of
include/mdvt_megasam.h, written from the header's formulas, and of the whole step around a tracker (tools/sam_track_video.py), run on
the test machine, never by the library.  Built on tests/mvsa_ref.py (torch's bilinear), tests/metric_align_ref.py (cv2's linear resize
on float32, the depth code) and tests/convergence_ref.py (OpenCV's 8-bit grey).  tests/test_megasam_cpu.py holds the restatements to
the exact box mean and to torch's CPU kernels.  Plain module: no fixture, no pytest setting."""
import numpy as np

import convergence_ref as cr
import metric_align_ref as mr
import mvsa_ref as mv

F = np.float32


# ---- mdvt_area_model_frames -------------------------------------------------------------------------------------------------------
def area_taps(ssize, dsize):
    """OpenCV's computeResizeAreaTab for one axis, restated -> [(first source sample, float32 weights)] per destination sample."""
    scale = ssize / dsize
    taps = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = int(np.ceil(f1)), min(int(np.floor(f2)), ssize - 1)
        s1 = min(s1, s2)
        first, w = s1, []
        if s1 - f1 > 1e-3:
            first = s1 - 1
            w.append((s1 - f1) / cell)
        w.extend([1.0 / cell] * (s2 - s1))
        if f2 - s2 > 1e-3:
            w.append(min(min(f2 - s2, 1.0), cell) / cell)
        taps.append((first, np.array(w, dtype=np.float64).astype(F)))
    return taps


def area_table(ssize, dsize):
    """-> (first int32 [dsize], count int32 [dsize], w float32 [dsize, ktaps], zero behind count): the table the library uploads."""
    taps = area_taps(ssize, dsize)
    ktaps = max(len(w) for _, w in taps)
    first = np.array([f for f, _ in taps], np.int32)
    count = np.array([len(w) for _, w in taps], np.int32)
    w = np.zeros((dsize, ktaps), F)
    for d, (_, a) in enumerate(taps):
        w[d, :len(a)] = a
    return first, count, w


def area_refusal(in_w, in_h, mid_w, mid_h):
    """The reason mdvt_area_model_frames refuses a size pair, or None."""
    if mid_w > in_w or mid_h > in_h:
        return "area enlargement is another algorithm"
    if in_w % mid_w == 0 and in_h % mid_h == 0 and (in_w, in_h) != (mid_w, mid_h):
        return "integer factors"
    return None


def area_planes(img, mid_size, crop_size=None):
    """One image [H, W, C] uint8 -> uint8 [hc, wc, C]: cv2.resize(INTER_AREA) to mid_size = (w1, h1), the top-left crop_size = (wc, hc).
    Every product and every sum is one float32 operation, the taps in ascending order."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    w1, h1 = int(mid_size[0]), int(mid_size[1])
    wc, hc = (w1, h1) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    why = area_refusal(W, H, w1, h1)
    if why:
        raise ValueError(why)
    xf, xn, xw = area_table(W, w1)
    yf, yn, yw = area_table(H, h1)
    xf, xn, xw, yf, yn, yw = xf[:wc], xn[:wc], xw[:wc], yf[:hc], yn[:hc], yw[:hc]
    src = img.astype(F)
    buf = np.zeros((H, wc) + img.shape[2:], F)                       # the horizontal sums of every source row
    for k in range(xw.shape[1]):                                    # (a tap behind count has weight 0 and adds +0: the sum stays as it is)
        buf = buf + src[:, np.minimum(xf + k, W - 1)] * xw[:, k].reshape((1, wc) + (1,) * (img.ndim - 2))
        assert buf.dtype == np.float32
    out = None
    for k in range(yw.shape[1]):
        t = yw[:, k].reshape((hc, 1) + (1,) * (img.ndim - 2)) * buf[np.minimum(yf + k, H - 1)]
        out = t if out is None else out + t
        assert out.dtype == np.float32
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def area_model_frames(rgb, mid_size, crop_size=None):
    """uint8 frames [N, H, W, 3] in R, G, B -> uint8 [N, 3, hc, wc]."""
    return np.stack([area_planes(f, mid_size, crop_size).transpose(2, 0, 1) for f in np.asarray(rgb, np.uint8)])


def box_mean(img, mid_size):
    """The exact box mean of an image [H, W, C] at mid_size = (w1, h1), in float64 from integer overlaps: what INTER_AREA approximates."""
    def weights(S, D):
        w = np.zeros((D, S))
        for d in range(D):
            for s in range(S):
                w[d, s] = max(0, min((d + 1) * S, (s + 1) * D) - max(d * S, s * D)) / S       # overlap of [d S, (d + 1) S] and [s D, (s + 1) D], in units of 1 / D
        return w
    img = np.asarray(img, np.float64)
    wy, wx = weights(img.shape[0], int(mid_size[1])), weights(img.shape[1], int(mid_size[0]))
    return np.einsum("ys,sxc,dx->ydc", wy, img, wx)


# ---- torch's nearest-exact map ----------------------------------------------------------------------------------------------------
def nex(n_in, n_out):
    """-> int64 [n_out]: torch's CPU nearest-exact source index of every output index."""
    scale = F(F(n_in) / F(n_out))
    f = np.floor(F(np.arange(n_out).astype(F) + F(0.5)) * scale)
    assert f.dtype == np.float32
    return np.minimum(f.astype(np.int64), n_in - 1)


def nex_planes(x, size):
    """planes [..., H, W] -> [..., h, w] at size = (w, h)."""
    return x[..., nex(x.shape[-2], int(size[1]))[:, None], nex(x.shape[-1], int(size[0]))[None, :]]


# ---- mdvt_tracker_depth, mdvt_tracker_mask ----------------------------------------------------------------------------------------
def _crop(x, mid_size, crop_size):
    wc, hc = (int(mid_size[0]), int(mid_size[1])) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    return x[..., :hc, :wc]


def tracker_depth(codes, max_depth, mid_size, crop_size=None):
    """uint8 depth frames [N, H, W, 3] in R, G, B -> float32 [N, hc, wc].  The green byte is not read."""
    codes = np.asarray(codes, np.uint8)
    u = (codes[..., 0].astype(np.uint32) << 24) | (codes[..., 2].astype(np.uint32) << 16)
    d = u.astype(F) / F((255 ** 4) / max_depth)
    assert d.dtype == np.float32
    return np.ascontiguousarray(_crop(nex_planes(d, mid_size), mid_size, crop_size))


def tracker_mask(masks, mid_size, crop_size=None):
    """uint8 mask frames [N, H, W, 3] in R, G, B -> float32 [N, hc, wc]."""
    v = (255 - cr.gray_of(np.asarray(masks, np.uint8)).astype(np.int64)).astype(F) / F(255)
    assert v.dtype == np.float32
    return np.ascontiguousarray(_crop(mv.bilinear_planes(v, mid_size), mid_size, crop_size))


# ---- mdvt_tracker_outputs ---------------------------------------------------------------------------------------------------------
def tracker_outputs(planes, mode, max_value, out_size, bgr=False):
    """float32 planes [N, h, w] -> uint8 frames [N, H, W, 3] at out_size = (W, H)."""
    planes = np.asarray(planes, F)
    W, H = int(out_size[0]), int(out_size[1])
    frames = []
    for p in planes:
        with np.errstate(all="ignore"):
            if mode == 0:
                d = nex_planes(p, (W, H))
                frames.append(mr.code(np.where(np.isnan(d), F(0), d), max_value, bgr)[1])
            else:
                if p.shape[1] == 2 * W and p.shape[0] == 2 * H:
                    raise ValueError("an exact 2 x reduction")
                d = mr.resize_linear(p, W, H)
                m = F(max_value)
                g = np.clip(d, 0, m) / m * F(255)
                assert g.dtype == np.float32
                b = np.where(np.isnan(g), F(0), g).astype(np.uint8)      # the decree: a NaN gives 0
                frames.append(np.stack([b, b, b], axis=-1))
    return np.stack(frames)


# ---- the whole step ---------------------------------------------------------------------------------------------------------------
def frame_plan(n_depth, n_color, n_mask, max_frames):
    """(frames handed over, the track_final frame or None) of stv:78-198 in closed form (the tool's own function follows the loop
    read by read; tests/test_megasam_cpu.py holds the two to each other)."""
    N, M = n_depth, max_frames
    if M != -1 and N >= M + 3:
        return M + 2, M + 1
    longer = n_color > N and (n_mask is None or n_mask > N)
    if not longer or (M != -1 and N == M + 2):
        return N - 1, None
    return N, N - 1


def model_size(h0, w0):
    h1 = int(h0 * np.sqrt((384 * 512) / (h0 * w0)))
    w1 = int(w0 * np.sqrt((384 * 512) / (h0 * w0)))
    return h1, w1, h1 - h1 % 8, w1 - w1 % 8


def pose_matrix(p):
    """One pose tx ty tz qx qy qz qw -> its 4 x 4 matrix [R | t] in float64."""
    tx, ty, tz, x, y, z, w = (float(v) for v in p)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = [tx, ty, tz]
    return T


def pose_inverse(p):
    """The decree's closed form of the inverse: [R^T | -R^T t]."""
    T = pose_matrix(p)
    inv = np.eye(4)
    inv[:3, :3] = T[:3, :3].T
    inv[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return inv


def run_step(color, depth, mask, core, *, max_frames=-1, max_depth=100, xfov=None, yfov=None):
    """The step on RGB frames [N, H, W, 3] (mask: None or frames) around core(items) -> (traj, depth_est, motion, intrinsics), the
    NumPy heart of a stub tracker -> dict(items: the tracker's inputs, final: the track_final index, transformations float64
    [t + 1, 4, 4], depth_frames and motion_frames uint8 [t, H, W, 3], intrinsics0)."""
    H, W = depth.shape[1:3]
    count, final = frame_plan(len(depth), len(color), None if mask is None else len(mask), max_frames)
    h1, w1, hc, wc = model_size(H, W)
    fx = W / (2 * np.tan(np.deg2rad(xfov) / 2)) if xfov is not None else None
    fy = H / (2 * np.tan(np.deg2rad(yfov) / 2)) if yfov is not None else None
    fx, fy = (fy if fx is None else fx), (fx if fy is None else fy)
    k = np.array([fx, fy, W / 2, H / 2], dtype=np.float64).astype(F)
    k[0::2] *= F(w1 / W)
    k[1::2] *= F(h1 / H)
    images = area_model_frames(color[:count], (w1, h1), (wc, hc))
    depths = tracker_depth(depth[:count], max_depth, (w1, h1), (wc, hc))
    masks = tracker_mask(mask[:count], (w1, h1), (wc, hc)) if mask is not None else np.ones_like(depths)
    items = [(i, images[i:i + 1], depths[i], k.copy(), masks[i]) for i in range(count)]
    traj, depth_est, motion, intr = core(items)
    T = np.stack([np.eye(4)] + [pose_inverse(p) for p in np.asarray(traj, np.float64)])
    return dict(items=items, final=final, transformations=T, intrinsics0=np.asarray(intr, F)[0],
                depth_frames=tracker_outputs(depth_est, 0, float(max_depth), (W, H)),
                motion_frames=tracker_outputs(motion, 1, 1.0, (W, H)))
