"""The expected values of the metric-alignment tests: compute_scale_and_shift_full, the per-pixel inverse with its two clean-up
rules, the bilinear resize and the 16-bit depth code as include/mdvt_metric_align.h states them, run by NumPy on the test machine,
never by the library.  cv2.resize(INTER_LINEAR) on float32 is restated from its tables (cv2 is not a dependency).  Also the input
generators of the tests and three models of a float32 sum's order.  Plain module: no fixture, no pytest setting."""
import numpy as np

F = np.float32


def same_bits(got, want):
    """Indices where two float32 arrays differ in their bits (so -0 is not +0); any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    return np.flatnonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


# ---- the fit --------------------------------------------------------------------------------------------------------------------
def five_arrays(prediction, target, mask=None):
    """The five float32 arrays whose sums the fit takes, each product rounded before the next."""
    prediction, target = np.ascontiguousarray(prediction, F), np.ascontiguousarray(target, F)
    mask = np.ones_like(prediction) if mask is None else np.ascontiguousarray(mask).astype(F)
    mp = mask * prediction
    return [mp * prediction, mp, mask, mp * target, mask * target]


def solve(a_00, a_01, a_11, b_0, b_1):
    with np.errstate(all="ignore"):
        det = F(F(a_00 * a_11) - F(a_01 * a_01))
        if det != 0:
            scale = F(F(F(a_11 * b_0) - F(a_01 * b_1)) / det)
            shift = F(F(F(-a_01 * b_0) + F(a_00 * b_1)) / det)
        else:
            scale, shift = F(1), F(0)
    return scale, shift, det


def fit(prediction, target, mask=None):
    """-> float32 [8]: a_00, a_01, a_11, b_0, b_1, scale, shift, det.  prediction and target: the frames concatenated along axis 0
    ([n_frames * H, W], or any contiguous shape: np.sum of a contiguous array does not depend on it)."""
    with np.errstate(all="ignore"):
        sums = [np.sum(a) for a in five_arrays(prediction, target, mask)]
        assert all(s.dtype == np.float32 for s in sums)
        return np.array(sums + list(solve(*sums)), F)


def concat(frames):
    """[N, H, W] -> the reference's np.concatenate of the frames: [N * H, W]."""
    frames = np.asarray(frames)
    return np.ascontiguousarray(frames.reshape(-1, frames.shape[-1]))


def pw(a):
    """NumPy's pairwise sum of a float32 sequence, every operation rounded to float32."""
    n = len(a)
    if n < 8:
        r = F(0)
        for x in a:
            r = F(r + x)
        return r
    if n <= 128:
        r = [a[k] for k in range(8)]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] = F(r[k] + a[i + k])
            i += 8
        res = F(F(F(r[0] + r[1]) + F(r[2] + r[3])) + F(F(r[4] + r[5]) + F(r[6] + r[7])))
        while i < n:
            res = F(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F(pw(a[:n2]) + pw(a[n2:]))


def sum_chunked(a):
    """The order this package reproduces: chunks of 8192 values, each summed pairwise, the chunk sums added in sequence."""
    a = np.ascontiguousarray(a, F).ravel()
    with np.errstate(all="ignore"):
        acc = F(0)
        for c in range(0, len(a), 8192):
            acc = F(acc + pw(a[c:c + 8192]))
    return acc


def sum_left_to_right(a):
    a = np.ascontiguousarray(a, F).ravel()
    with np.errstate(all="ignore"):
        return np.cumsum(a, dtype=F)[-1]                            # (an accumulation cannot be reordered)


def sum_f64_rounded(a):
    with np.errstate(all="ignore"):
        return F(np.sum(np.ascontiguousarray(a, F).ravel().astype(np.float64)))


def orders_told_apart(prediction, target, mask=None):
    """(some sum differs between NumPy's order and a left-to-right sum, some sum differs between NumPy's order and float64)."""
    arrays = five_arrays(prediction, target, mask)
    ours = [np.sum(a) for a in arrays]
    return (any(o.tobytes() != sum_left_to_right(a).tobytes() for o, a in zip(ours, arrays)),
            any(o.tobytes() != sum_f64_rounded(a).tobytes() for o, a in zip(ours, arrays)))


# ---- the inputs of the fit tests --------------------------------------------------------------------------------------------------
def gen_model(rng, N, H, W):
    """Predictions in (0, 3], metric depth in [0.3, 80]: -> (prediction, depth)."""
    p = (F(3) - rng.random((N, H, W), dtype=F) * F(3)).astype(F)
    p[p <= 0] = F(3)
    d = (F(0.3) + rng.random((N, H, W), dtype=F) * F(79.7)).astype(F)
    return p, d


def gen_spread(rng, N, H, W):
    """Magnitudes spread over 1e-3 ... 1e3, both signs in the prediction: -> (prediction, depth)."""
    p = (10.0 ** rng.uniform(-3, 3, (N, H, W)) * rng.choice([-1.0, 1.0], (N, H, W), p=(0.2, 0.8))).astype(F)
    d = (10.0 ** rng.uniform(-3, 3, (N, H, W))).astype(F)
    return p, d


def gen_relative(rng, N, H, W):
    """A relative inverse depth: affine in 1 / depth, plus noise: -> (prediction, depth)."""
    d = gen_model(rng, N, H, W)[1]
    p = (F(1) / d * F(2.5) + F(0.07) + rng.normal(0, 0.01, d.shape).astype(F)).astype(F)
    return p, d


def gen_mask(rng, N, H, W, values=(0, 1, 3)):
    return rng.choice(np.array(values, np.uint8), (N, H, W))


GENERATORS = {"model": gen_model, "spread": gen_spread, "relative": gen_relative}


def fit_input(gen, shape, seed):
    """-> (prediction, depth, mask uint8 of 0, 1 and 3): the arrays of one fit test, the same wherever they are drawn."""
    rng = np.random.default_rng(seed)
    p, d = GENERATORS[gen](rng, *shape)
    return p, d, gen_mask(rng, *shape)


# Every (generator, shape, seed) the GPU fit tests (tests/test_gpu_metric_align.py) draw with fit_input, by test.  The condition on
# them (tests/test_metric_align_cpu.py) is checked on these very arrays.
# element totals 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 2 * 8192, 3 * 8192 + 1003 and 32 x 98 x 174, and three more whose
# chunks and leaves straddle rows and frames
FIT_SHAPES = [(1, 1, 1), (1, 1, 7), (2, 2, 2), (1, 3, 3), (1, 1, 127), (2, 64, 1), (1, 3, 43), (1, 1, 8191), (2, 64, 64), (1, 2731, 3),
              (2, 8192, 1), (1, 1, 3 * 8192 + 1003), (32, 98, 174), (3, 37, 53), (1, 61, 67), (5, 41, 83)]
VECTOR_SHAPES = [(2, 64, 64), (3, 36, 52), (5, 40, 84), (32, 96, 172)]           # widths that are multiples of 4
GROWTH_SHAPES = [(1, 3, 43), (5, 41, 83), (2, 2053, 2047)]                       # the last: 1026 chunks, two launch sets
FIT_INPUTS = {
    "every_size": [("model", s, sum(s) * 37 + s[2]) for s in FIT_SHAPES],
    "vector": [("spread", s, sum(s)) for s in VECTOR_SHAPES],
    "value_sets": [("spread", (3, 37, 53), 53), ("model", (3, 37, 53), 54), ("model", (3, 37, 53), 55), ("model", (3, 37, 53), 56)],
    "side_stream": [("model", (5, 41, 83), 83)],
    "growth": [("model", s, 1026 + k) for k, s in enumerate(GROWTH_SHAPES)],
    "refusals": [("model", (3, 6, 20), 6)],
    "codes_behind_a_fit": [("relative", (4, 37, 53), 96)],
}


def inverse(depth):
    with np.errstate(all="ignore"):
        return (F(1) / np.asarray(depth, F)).astype(F)


# ---- reconstruction, resize, code ---------------------------------------------------------------------------------------------------
def reconstruct(x, scale, shift, max_depth, style):
    x, scale, shift = np.asarray(x, F), F(scale), F(shift)
    with np.errstate(all="ignore"):
        inv = (x * scale) + shift
        assert inv.dtype == np.float32
        if style == 0:
            d = F(1) / inv
            d[d < 0.0] = float(max_depth)
            return d
        inv[inv == 0.0] = 1e-4
        d = np.clip(F(1) / inv, 0, max_depth)
        return np.where(np.isnan(d), F(max_depth), d).astype(F)      # (nan_to_num's nan=; nothing is infinite after the clip)


def linear_table(n_in, n_out):
    """-> (s0 int [n_out], s1 int [n_out], w0 float32 [n_out], w1 float32 [n_out]) of cv2's INTER_LINEAR along one axis."""
    s0, s1, w0, w1 = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros(n_out, F), np.zeros(n_out, F)
    ratio = n_in / n_out
    for d in range(n_out):
        f = F((d + 0.5) * ratio - 0.5)
        s = int(np.floor(f))
        f = F(f - F(s))
        if s < 0:
            s, f = 0, F(0)
        if s >= n_in - 1:
            s, f = n_in - 1, F(0)
        s0[d], s1[d], w0[d], w1[d] = s, min(s + 1, n_in - 1), F(F(1) - f), f
    return s0, s1, w0, w1


def resize_linear(d, out_w, out_h):
    """cv2.resize(d, (out_w, out_h), INTER_LINEAR) of a float32 plane [H, W], restated: horizontal pass, then vertical."""
    d = np.asarray(d, F)
    h, w = d.shape
    if (w, h) == (out_w, out_h):
        return d
    x0, x1, a0, a1 = linear_table(w, out_w)
    y0, y1, b0, b1 = linear_table(h, out_h)
    with np.errstate(all="ignore"):
        r = d[:, x0] * a0[None, :] + d[:, x1] * a1[None, :]
        out = r[y0] * b0[:, None] + r[y1] * b1[:, None]
    assert out.dtype == np.float32
    return out


def code(d, max_depth, bgr=False):
    """-> (c float32 [H, W], uint8 [H, W, 3]): encode_depth_as_uint32 + encode_data_as_BGR(bit16=True)."""
    c = np.clip(np.asarray(d, F), 0, max_depth)
    assert c.dtype == np.float32
    with np.errstate(all="ignore"):
        u = ((255 ** 4 / float(max_depth)) * c.astype(np.float64)).astype(np.uint32)
    hi, lo = (u >> 24).astype(np.uint8), ((u >> 16) & 0xFF).astype(np.uint8)
    return c, np.stack([lo, hi, hi] if bgr else [hi, hi, lo], axis=-1)


def metric_codes(x, scale, shift, max_depth, style, out_size=None, bgr=False):
    """relative planes [N, H, W] -> (codes uint8 [N, H', W', 3], depth float32 [N, H', W'])."""
    codes, depths = [], []
    for plane in np.asarray(x, F):
        d = reconstruct(plane, scale, shift, max_depth, style)
        if out_size is not None:
            d = resize_linear(d, int(out_size[0]), int(out_size[1]))
            if style == 1 and d.shape != plane.shape:
                d = np.clip(d, 0, max_depth)
        c, rgb = code(d, max_depth, bgr)
        codes.append(rgb)
        depths.append(c)
    return np.stack(codes), np.stack(depths)
