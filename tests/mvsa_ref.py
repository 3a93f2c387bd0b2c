"""The expected values of the MVSAnywhere step's tests: NumPy restatements of the three entry points of include/mdvt_mvsa.h, written from
the header's formulas, and of the whole step around a model (tools/video_mvsa.py), run on the test machine, never by the library.
tests/test_mvsa_cpu.py holds the restatements to torch's CPU kernels.  Plain module: no fixture, no pytest setting."""
import numpy as np

import metric_align_ref as mr

F = np.float32


# ---- mdvt_bilinear_model_frames ---------------------------------------------------------------------------------------------------
def linear_axis(n_in, n_out):
    """-> (i0, i1 int64 [n_out], w0, w1 float32 [n_out]): the header's per-axis formula, every operation one float32 operation."""
    scale = F(F(n_in) / F(n_out))
    x = np.arange(n_out).astype(F)
    src = F(scale * F(x + F(0.5))) - F(0.5)
    assert src.dtype == np.float32
    src = np.maximum(src, F(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = np.minimum(np.maximum(src - i0.astype(F), F(0)), F(1))
    assert lam.dtype == np.float32
    return i0, i1, F(1) - lam, lam


def bilinear_planes(v, out_size):
    """float32 planes [..., H, W] -> [..., h, w] at out_size = (w, h): horizontally on the two source rows, then vertically; where
    w + h <= 128 the four-weight form, as torch's CPU dispatch chooses between its two kernels."""
    v = np.asarray(v, F)
    w, h = int(out_size[0]), int(out_size[1])
    x0, x1, wx0, wx1 = linear_axis(v.shape[-1], w)
    y0, y1, wy0, wy1 = linear_axis(v.shape[-2], h)
    if w + h <= 128:                                                # torch's kernel for small outputs: four weights, summed in order
        b0, b1 = wy0[:, None], wy1[:, None]
        r0, r1 = v[..., y0, :], v[..., y1, :]
        out = (((b0 * wx0) * r0[..., x0] + (b0 * wx1) * r0[..., x1]) + (b1 * wx0) * r1[..., x0]) + (b1 * wx1) * r1[..., x1]
        assert out.dtype == np.float32
        return out
    t = wx0 * v[..., x0] + wx1 * v[..., x1]                        # [..., H, w]: every product rounded, then the sum
    assert t.dtype == np.float32
    out = wy0[:, None] * t[..., y0, :] + wy1[:, None] * t[..., y1, :]
    assert out.dtype == np.float32
    return out


def bilinear_model_frames(rgb, out_size=None):
    """uint8 frames [N, H, W, 3] in R, G, B -> float32 [N, 3, h, w]."""
    rgb = np.asarray(rgb, np.uint8)
    v = rgb.transpose(0, 3, 1, 2).astype(F) / F(255)
    assert v.dtype == np.float32
    return bilinear_planes(v, (rgb.shape[2], rgb.shape[1]) if out_size is None else out_size)


def bilinear_bound(in_w, in_h):
    """B of the step's tests against torch: a unit in the last place of the source index per axis times a value range of 1 (what a
    contracted index costs), and four roundings."""
    return 2.0 ** (int(np.ceil(np.log2(in_w))) - 24) + 2.0 ** (int(np.ceil(np.log2(in_h))) - 24) + 4 * 2.0 ** -24


# ---- the nearest map ------------------------------------------------------------------------------------------------------------
def near(n_in, n_out):
    """-> int64 [n_out]: torch's CPU nearest source index of every output index."""
    scale = F(F(n_in) / F(n_out))
    f = np.floor(np.arange(n_out).astype(F) * scale)
    assert f.dtype == np.float32
    return np.minimum(f.astype(np.int64), n_in - 1)


def near_twice(n_in, n_mid, n_out):
    return near(n_in, n_mid)[near(n_mid, n_out)]


def nearest_planes(x, size):
    """planes [..., H, W] -> [..., h, w] at size = (w, h) through one nearest map."""
    return x[..., near(x.shape[-2], int(size[1]))[:, None], near(x.shape[-1], int(size[0]))[None, :]]


# ---- mdvt_nearest_depth_codes -----------------------------------------------------------------------------------------------------
def nearest_depth_codes(x, mid_size, out_size, max_depth, scales=None, bgr=False):
    """float32 planes [N, H, W] -> (codes uint8 [N, h, w, 3], c float32 [N, h, w]).  scales: None, or one float32 factor per frame."""
    x = np.asarray(x, F)
    sy = near_twice(x.shape[1], int(mid_size[1]), int(out_size[1]))
    sx = near_twice(x.shape[2], int(mid_size[0]), int(out_size[0]))
    codes, planes = [], []
    for k, plane in enumerate(x):
        d = plane[sy[:, None], sx[None, :]]
        with np.errstate(all="ignore"):
            if scales is not None:
                d = d * F(np.asarray(scales, F).reshape(-1)[k])
            assert d.dtype == np.float32
            c, rgb = mr.code(np.where(np.isnan(d), F(0), d), max_depth, bgr)
        codes.append(rgb)
        planes.append(np.where(np.isnan(d), d, c))                  # a NaN has code 0 and stays in the plane
    return np.stack(codes), np.stack(planes)


# ---- mdvt_ratio_median ------------------------------------------------------------------------------------------------------------
def valid_ratios(cv, ref, mask=None):
    """One frame: cv [h_cv, w_cv], ref [h_ref, w_ref], mask uint8 [h_m, w_m] or None -> the valid ratios, float32, in row-major order."""
    cv, ref = np.asarray(cv, F), np.asarray(ref, F)
    size = (cv.shape[1], cv.shape[0])
    ref_at = nearest_planes(ref, size)
    m = np.ones(cv.shape, bool) if mask is None else nearest_planes(np.asarray(mask), size) != 0
    with np.errstate(all="ignore"):
        valid = m & np.isfinite(cv) & np.isfinite(ref_at) & (cv > 0) & (ref_at > 0)
        ratio = np.maximum(cv[valid] / (ref_at[valid] + F(1e-6)), F(0))
    assert ratio.dtype == np.float32
    return ratio


def ratio_median(cv, ref, mask=None):
    """frames [N, ...] -> (medians float32 [N], counts uint32 [N]): the lower median, 1.0 where nothing is valid."""
    med, cnt = [], []
    for k in range(len(cv)):
        r = np.sort(valid_ratios(cv[k], ref[k], None if mask is None else mask[k]))
        cnt.append(r.size)
        med.append(r[(r.size - 1) // 2] if r.size else F(1))
    return np.array(med, F), np.array(cnt, np.uint32)


# ---- the step ---------------------------------------------------------------------------------------------------------------------
def reference_indices(i, n, window):
    """video_mvsa.py:146-161 as the plain loop."""
    half_w = max(1, window // 2)
    ref = []
    for d in range(-half_w, half_w + 1):
        j = i + d
        if j < 0 or j >= n or j == i:
            continue
        ref.append(j)
    if len(ref) == 0:
        ref = [min(n - 1, max(0, i + 1))]
    return ref


def run_step(frames, infer, *, resize_w, window, max_depth, apply_scale=False):
    """The whole step on host arrays.  frames uint8 [n, H, W, 3] in R, G, B; infer(image [3, h, w], refs [R, 3, h, w], i, ref_idx) ->
    (depth [h_ref, w_ref], lowest_cost [h_cv, w_cv], mask uint8 [h_m, w_m] or None) in NumPy.
    -> (codes [n, H, W, 3] in R, G, B, the frames' median ratios float32 [n])."""
    n, H, W = frames.shape[:3]
    scale = resize_w / float(W)
    size = (int(round(W * scale)), int(round(H * scale)))
    planes = bilinear_model_frames(frames, size)
    codes, scales = [], []
    for i in range(n):
        ref_idx = reference_indices(i, n, window)
        depth, cv, mask = infer(planes[i], planes[ref_idx], i, ref_idx)
        depth, cv = np.asarray(depth, F), np.asarray(cv, F)
        s, _ = ratio_median(cv[None], depth[None], None if mask is None else np.asarray(mask)[None])
        scales.append(s[0])
        codes.append(nearest_depth_codes(depth[None], (cv.shape[1], cv.shape[0]), (W, H), max_depth, s if apply_scale else None)[0][0])
    return np.stack(codes), np.array(scales, F)
