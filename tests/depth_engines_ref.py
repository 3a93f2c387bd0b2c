"""The expected values of the depth-engine tests: NumPy restatements of the three entry points of include/mdvt_depth_engines.h, written
from the header's text and run on the test machine, never by the library, and of the two steps around a model
(tools/depth_engine_video.py, tools/upscale_depth_promptda.py) from the frames to the codes and the x-fov list.  Built on the pieces
other restatements already hold to their references: infill_adapter_ref.resize_u8 (the u8 resize), metric_align_ref.linear_table /
resize_linear (the float32 resize) and metric_align_ref.pw / sum_chunked (NumPy's order of summation).  tests/golden/depth_engines.npz
holds the focal estimate's values, selections and means to the reference's own function (tests/test_depth_engines_cpu.py).
Plain module: no fixture, no pytest setting."""
import math

import numpy as np

import depth_sink_ref as dr
import infill_adapter_ref as iar
import metric_align_ref as mr

F = np.float32
EPS = F(1e-6)


# ---- mdvt_model_frames ----------------------------------------------------------------------------------------------------------
def model_frames(frames, out_size=None, as_float=False, bgr=False):
    """uint8 [N, H, W, 3] -> [N, 3, h, w] in R, G, B plane order: uint8, or float32 v / 255 (one division)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    H, W = frames.shape[1:3]
    w, h = (W, H) if out_size is None else (int(out_size[0]), int(out_size[1]))
    out = np.stack([iar.resize_u8(f, w, h) for f in frames])
    if bgr:
        out = out[..., ::-1]
    out = np.ascontiguousarray(out.transpose(0, 3, 1, 2))
    if not as_float:
        return out
    out = out.astype(F) / F(255)
    assert out.dtype == np.float32
    return out


# ---- mdvt_depth_prompt ----------------------------------------------------------------------------------------------------------
def decode(codes, max_depth, bgr=False):
    """dfh:21-23 on uint8 [..., 3]: float32(R << 24 | B << 16) * float32(max_depth / 255^4)."""
    codes = np.asarray(codes)
    R, B = (codes[..., 2], codes[..., 0]) if bgr else (codes[..., 0], codes[..., 2])
    e = ((R.astype(np.uint32) << 24) | (B.astype(np.uint32) << 16)).astype(F)
    d = e * F(float(max_depth) / 255 ** 4)
    assert d.dtype == np.float32
    return d


def depth_prompt(codes, max_depth, out_size, bgr=False):
    """uint8 [N, H, W, 3] -> float32 [N, h, w]: the decode, then cv2.resize(INTER_LINEAR) on float32 as restated."""
    w, h = int(out_size[0]), int(out_size[1])
    return np.stack([mr.resize_linear(decode(f, max_depth, bgr), w, h) for f in np.asarray(codes)])


# ---- mdvt_focal_from_points -----------------------------------------------------------------------------------------------------
def channel_last(points):
    """[N, H, W, 3] or [N, 3, H, W] -> [N, H, W, 3], a last dimension of 3 read as the former (unik3d_video.py:46-52)."""
    points = np.asarray(points, F)
    assert points.ndim == 4
    return points if points.shape[-1] == 3 else points.transpose(0, 2, 3, 1)


def focal_values(points):
    """One frame [H, W, 3] -> (ex, ey float32 [H, W], mx, my bool [H, W]): unik3d_video.py:82-95, each step in float32."""
    points = np.asarray(points, F)
    H, W = points.shape[:2]
    X, Y, Z = points[..., 0], points[..., 1], points[..., 2]
    v, u = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        z_ok = np.abs(Z) > EPS
        mx, my = (np.abs(X) > EPS) & z_ok, (np.abs(Y) > EPS) & z_ok
        ex = (u.astype(F) - F(W / 2.0)) * (Z / X)
        ey = (v.astype(F) - F(H / 2.0)) * (Z / Y)
    assert ex.dtype == np.float32 and ey.dtype == np.float32
    return ex, ey, mx, my


def mean_selected(e, m, total=np.sum):
    """The float32 mean of e[m] in row-major order, 0.0 where nothing is selected.  total: np.sum, whose order on a contiguous float32
    array is the one the header names, or metric_align_ref.sum_chunked, that order spelled out (slow: a Python loop)."""
    sel = np.ascontiguousarray(e[m], F)
    if sel.size == 0:
        return F(0.0)
    with np.errstate(all="ignore"):
        return F(F(total(sel)) / F(sel.size))


def focal(points, total=np.sum):
    """[N, H, W, 3] or [N, 3, H, W] -> (float32 [N, 2] = (fx, fy), int64 [N, 2] = (nx, ny))."""
    f, n = [], []
    for p in channel_last(points):
        ex, ey, mx, my = focal_values(p)
        f.append([mean_selected(ex, mx, total), mean_selected(ey, my, total)])
        n.append([int(mx.sum()), int(my.sum())])
    return np.array(f, F), np.array(n, np.int64)


# ---- the x-fov, per script (fov_from_camera_matrix, dmt:1640-1649) --------------------------------------------------------------------
def xfov_f64(fx, width):
    """float64: cx = width / 2; rad2deg(2 * arctan2(2 cx, 2 fx))."""
    return float(np.rad2deg(2 * np.arctan2(np.float64(width / 2) * 2, 2 * np.float64(fx))))


def xfov_f32(K):
    K = np.asarray(K, F)
    return float(np.rad2deg(F(F(2) * np.arctan2(F(K[0][2] * F(2)), F(F(2) * K[0][0])))))


def closest_higher_multiple(x, base=14):
    return math.ceil(x / base) * base


# ---- the steps ------------------------------------------------------------------------------------------------------------------
def run_engine(frames, engine, infer, max_depth, batch):
    """frames uint8 [n, H, W, 3] RGB, infer(planar frames of a batch) -> the engine's dict of NumPy arrays -> (codes uint8
    [n, H, W, 3], xfovs)."""
    n, H, W = frames.shape[:3]
    codes, xfovs = [], []
    for a in range(0, n, batch):
        got = infer(model_frames(frames[a:a + batch], as_float=engine == "moge"))
        if engine == "unik3d":
            xfovs += [xfov_f64(F(fx), W) for fx, _ in focal(got["points"])[0]]
        elif engine == "moge":
            xfovs += [xfov_f32(K) for K in got["intrinsics"]]
        else:
            xfovs += [xfov_f64(float(f), W) for f in got["focallength_px"]]
        codes.append(dr.sink(got["depth"], max_depth, (W, H), nan_to_max=engine == "moge")[0])
    return np.concatenate(codes), xfovs


def run_promptda(color, depth_codes, upscale, max_depth, batch):
    """color, depth_codes uint8 [n, ., ., 3], upscale(rgb [k, 3, h14, w14], prompt [k, 1, 192, 256]) -> NumPy [k, h14, w14] -> codes
    uint8 [n, H, W, 3]."""
    n, H, W = color.shape[:3]
    size14 = (closest_higher_multiple(W), closest_higher_multiple(H))
    out = []
    for a in range(0, n, batch):
        rgb = model_frames(color[a:a + batch], size14, as_float=True)
        prompt = depth_prompt(depth_codes[a:a + batch], max_depth, (256, 192))[:, None]
        out.append(dr.sink(upscale(rgb, prompt), max_depth, (W, H))[0])
    return np.concatenate(out)
