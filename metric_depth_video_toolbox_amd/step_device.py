"""The device wrappers of the model-step tools (tools/video_da3.py, depth_engine_video.py, upscale_depth_promptda.py,
generate_video_mask.py, video_mvsa.py and scene_detect.py): the eleven functions that hand a tensor's address to the entry points of
include/mdvt_depth_sink.h, mdvt_depth_engines.h, mdvt_video_mask.h, mdvt_mvsa.h and mdvt_scene.h.  Each takes the clip's context
first, refuses a tensor its docstring does not promise to take before the library sees an address (tests/binding_contract.py holds
every one to its record), and only enqueues on `stream`.  torch is imported inside the functions: importing this module, or a tool,
needs none.  on_context and frames_on_context are also megasam_device.py's and inspatio_device.py's.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .step_clip import non_empty, size_arg, stream_or_current


def on_context(ctx, name: str, t):
    """The device of a checked tensor, which must be the context's (ffv1_device.enqueue's refusal)."""
    if t.device.index != ctx.device:
        raise ValueError(f"{name} is on {t.device}, the context on cuda:{ctx.device}")
    return t.device


def frames_on_context(ctx, name: str, frames, noun: str = "pixel", ndim=4):
    """A packed uint8 frame batch [N, H, W, 3] (rows and frames at any pitch, none overlapping) on the context's GPU, checked ->
    (device, N, H, W).  ndim=None words a wrong number of dimensions as a wrong shape."""
    import torch
    _lib.check_tensor(name, frames, torch.uint8, (None, None, None, 3), ndim=ndim, packed=2, disjoint=True)
    return (on_context(ctx, name, frames),) + non_empty(name, frames, noun)


# ---- include/mdvt_depth_sink.h ------------------------------------------------------------------------------------------------------

def depth_video_codes(ctx, planes, max_depth, out_size=None, *, scale=None, nan_to_max=False, bgr=False, want_plane=False, out=None,
                      stream=None):
    """mdvt_depth_video_codes on float32 CUDA planes [N, h, w] (rows and frames may be strided) -> the uint8 [N, H, W, 3] codes of a
    depth video at out_size = (W, H) (default: the planes' own size), R, G, B order (B, G, R with bgr).  scale: a one-element float32
    CUDA tensor every value is multiplied by first, read on the device; nan_to_max: NaN becomes max_depth before that.  want_plane:
    also the float32 [N, H, W] planes of the coded depth.  out: the codes' tensor to fill.  Only enqueues, on `stream`."""
    import torch
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    _lib.check_tensor("planes", planes, torch.float32, ndim=3, packed=1, disjoint=True)
    dev = on_context(ctx, "planes", planes)
    N, h, w = non_empty("planes", planes, "value")
    W, H = (w, h) if out_size is None else size_arg(out_size, "out_size")
    if scale is not None:
        _lib.check_tensor("scale", scale, torch.float32, device=dev, contiguous=True)
        if scale.numel() != 1:
            raise ValueError(f"scale must hold one value, got shape {tuple(scale.shape)}")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        codes = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) if out is None else out
        plane = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_plane else None
    _lib.check_tensor("out", codes, torch.uint8, (N, H, W, 3), device=dev, packed=2, output=True)
    ctx.call("mdvt_depth_video_codes", w, h, N, planes.data_ptr(), 4 * planes.stride(1), 4 * planes.stride(0),
             scale.data_ptr() if scale is not None else None, int(bool(nan_to_max)), float(max_depth), W, H,
             codes.data_ptr(), codes.stride(1), codes.stride(0), int(bool(bgr)),
             plane.data_ptr() if want_plane else None, 4 * W, 4 * W * H, _lib.stream_arg(dev, s))
    return (codes, plane) if want_plane else codes


# ---- include/mdvt_depth_engines.h ---------------------------------------------------------------------------------------------------

def model_frames(ctx, frames, out_size=None, *, as_float=False, bgr=False, stream=None):
    """mdvt_model_frames on uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided; B, G, R with bgr) -> the planar tensor
    [N, 3, h, w] in R, G, B plane order at out_size = (w, h) (default: the frames' own size), uint8, or float32 v / 255 with as_float.
    Only enqueues, on `stream`."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "frames", frames, ndim=None)
    w, h = (W, H) if out_size is None else size_arg(out_size, "out_size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, 3, h, w), dtype=torch.float32 if as_float else torch.uint8, device=dev)
    e = out.element_size()
    ctx.call("mdvt_model_frames", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w, h, int(bool(as_float)),
             out.data_ptr(), e * w, e * w * h, e * w * h * 3, _lib.stream_arg(dev, s))
    return out


def depth_prompt(ctx, codes, max_depth, out_size, *, bgr=False, stream=None):
    """mdvt_depth_prompt on uint8 CUDA depth frames [N, H, W, 3] (R, G, B; B, G, R with bgr; rows and frames may be strided) ->
    float32 [N, h, w] at out_size = (w, h): the decoded depth, resized like cv2.resize(INTER_LINEAR).  Only enqueues, on `stream`."""
    import torch
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    dev, N, H, W = frames_on_context(ctx, "codes", codes, ndim=None)
    w, h = size_arg(out_size, "out_size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, h, w), dtype=torch.float32, device=dev)
    ctx.call("mdvt_depth_prompt", W, H, N, codes.data_ptr(), codes.stride(1), codes.stride(0), int(bool(bgr)), float(max_depth), w, h,
             out.data_ptr(), 4 * w, 4 * w * h, _lib.stream_arg(dev, s))
    return out


def focal_from_points(ctx, points, *, want_counts=False, stream=None):
    """mdvt_focal_from_points on float32 CUDA point maps [N, H, W, 3] or [N, 3, H, W] (a last dimension of 3 is read as the
    former, as u3d:46-52 reads it; rows, planes and frames may be strided) -> float32 [N, 2] = (fx, fy) per frame and, with
    want_counts, the int32 tensor [N, 2] = (nx, ny) of the library's uint32 counts (at most 2^28 each).  Only enqueues, on `stream`."""
    import torch
    _lib.check_tensor("points", points, torch.float32, ndim=4)
    if points.shape[-1] == 3:
        _lib.check_tensor("points", points, torch.float32, ndim=4, packed=2, disjoint=True)
        layout, dims = 1, points.shape[:3]
        pitch, plane, stride = 4 * points.stride(1), 0, 4 * points.stride(0)
    elif points.shape[1] == 3:
        _lib.check_tensor("points", points, torch.float32, ndim=4, packed=1, disjoint=True)
        layout, dims = 0, (points.shape[0], *points.shape[2:])
        pitch, plane, stride = 4 * points.stride(2), 4 * points.stride(1), 4 * points.stride(0)
    else:
        raise ValueError(f"points must be [N, H, W, 3] or [N, 3, H, W], got shape {tuple(points.shape)}")
    dev = on_context(ctx, "points", points)
    N, H, W = non_empty("points", points, "point", dims)
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        focal = torch.empty((N, 2), dtype=torch.float32, device=dev)
        counts = torch.empty((N, 2), dtype=torch.int32, device=dev) if want_counts else None
    ctx.call("mdvt_focal_from_points", W, H, N, points.data_ptr(), layout, pitch, plane, stride, focal.data_ptr(),
             counts.data_ptr() if want_counts else None, _lib.stream_arg(dev, s))
    return (focal, counts) if want_counts else focal


# ---- include/mdvt_video_mask.h ------------------------------------------------------------------------------------------------------

def lanczos_resize(ctx, images, out_size, *, form=0, stream=None):
    """mdvt_lanczos_resize_u8 on uint8 CUDA images [N, H, W] (mode L) or [N, H, W, 3] (rows and frames may be strided) -> (the images
    at out_size = (w, h): Image.resize(out_size, LANCZOS) byte for byte, the form the call took: _lib.LANCZOS_FUSED,
    _lib.LANCZOS_TWO_LAUNCH or 0 for a copy).  Only enqueues, on `stream`."""
    import torch
    _lib.check_tensor("images", images, torch.uint8, ndim=(3, 4))
    ch = 1 if images.dim() == 3 else 3
    _lib.check_tensor("images", images, torch.uint8, (None, None, None) + ((3,) if ch == 3 else ()), packed=2 if ch == 3 else 1, disjoint=True)
    dev = on_context(ctx, "images", images)
    N, H, W = non_empty("images", images, "pixel")
    w, h = size_arg(out_size, "out_size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device=dev)
    took = C.c_int(-1)
    ctx.call("mdvt_lanczos_resize_u8", W, H, ch, N, images.data_ptr(), images.stride(1), images.stride(0), w, h,
             out.data_ptr(), ch * w, ch * w * h, int(form), C.cast(C.byref(took), C.c_void_p), _lib.stream_arg(dev, s))
    return out, int(took.value)


def mask_model_input(ctx, frames, model_size, mean, std, *, bgr=False, stream=None):
    """mdvt_mask_model_input on uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided; B, G, R with bgr) -> float32
    [N, 3, h, w] at model_size = (w, h), planes R, G, B: rembg's normalize.  Only enqueues, on `stream`."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "frames", frames, ndim=None)
    w, h = size_arg(model_size, "model_size")
    d3 = C.c_double * 3
    h_mean, h_std = d3(*(float(v) for v in mean)), d3(*(float(v) for v in std))
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, 3, h, w), dtype=torch.float32, device=dev)
    ctx.call("mdvt_mask_model_input", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w, h,
             C.cast(h_mean, C.c_void_p), C.cast(h_std, C.c_void_p), out.data_ptr(), 4 * w, 4 * w * h, 12 * w * h, _lib.stream_arg(dev, s))
    return out


def mask_from_prediction(ctx, pred, out_size, *, channels=3, stream=None):
    """mdvt_mask_from_prediction on float32 CUDA planes [N, h, w] (rows and frames may be strided) -> uint8 [N, H, W, 3] (three equal
    bytes: the mask video's frame) or, with channels=1, [N, H, W] at out_size = (W, H).  Only enqueues, on `stream`."""
    import torch
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels!r}")
    _lib.check_tensor("pred", pred, torch.float32, (None, None, None), packed=1, disjoint=True)
    dev = on_context(ctx, "pred", pred)
    N, ph, pw = non_empty("pred", pred, "value")
    W, H = size_arg(out_size, "out_size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, H, W) + ((3,) if channels == 3 else ()), dtype=torch.uint8, device=dev)
    ctx.call("mdvt_mask_from_prediction", pw, ph, N, pred.data_ptr(), 4 * pred.stride(1), 4 * pred.stride(0), W, H, int(channels),
             out.data_ptr(), channels * W, channels * W * H, _lib.stream_arg(dev, s))
    return out


# ---- include/mdvt_mvsa.h ------------------------------------------------------------------------------------------------------------

def bilinear_model_frames(ctx, frames, out_size=None, *, bgr=False, out=None, stream=None):
    """mdvt_bilinear_model_frames on uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided; B, G, R with bgr) -> the float32
    planar tensor [N, 3, h, w] in R, G, B plane order at out_size = (w, h) (default: the frames' own size): v / 255 through torch's
    bilinear resize, unfused.  out: the tensor to fill (rows, planes and frames may be strided).  Only enqueues, on `stream`."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "frames", frames, ndim=None)
    w, h = (W, H) if out_size is None else size_arg(out_size, "out_size")
    s = stream_or_current(dev, stream)
    if out is None:
        with torch.cuda.stream(s):
            out = torch.empty((N, 3, h, w), dtype=torch.float32, device=dev)
    _lib.check_tensor("out", out, torch.float32, (N, 3, h, w), device=dev, packed=1, output=True)
    ctx.call("mdvt_bilinear_model_frames", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w, h,
             out.data_ptr(), 4 * out.stride(2), 4 * out.stride(1), 4 * out.stride(0), _lib.stream_arg(dev, s))
    return out


def nearest_depth_codes(ctx, planes, mid_size, max_depth, out_size, *, scale=None, bgr=False, want_plane=False, out=None, stream=None):
    """mdvt_nearest_depth_codes on float32 CUDA planes [N, h, w] (rows and frames may be strided) -> the uint8 [N, H, W, 3] codes of a
    depth video at out_size = (W, H), sampled through two nearest maps, first to mid_size = (w_cv, h_cv).  scale: a float32 CUDA tensor
    of one factor for all frames or of N, read on the device.  want_plane: also the float32 [N, H, W] planes of the coded depth.
    out: the codes' tensor to fill.  Only enqueues, on `stream`."""
    import torch
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    _lib.check_tensor("planes", planes, torch.float32, ndim=3, packed=1, disjoint=True)
    dev = on_context(ctx, "planes", planes)
    N, h, w = non_empty("planes", planes, "value")
    (mw, mh), (W, H) = (int(v) for v in mid_size), (int(v) for v in out_size)
    if min(mw, mh, W, H) < 1:
        raise ValueError(f"mid_size and out_size must be (width, height) with both at least 1, got {mid_size!r}, {out_size!r}")
    scale_stride = 0
    if scale is not None:
        _lib.check_tensor("scale", scale, torch.float32, device=dev, contiguous=True)
        if scale.numel() not in (1, N):
            raise ValueError(f"scale must hold one value or one per frame, got shape {tuple(scale.shape)}")
        scale_stride = 4 if scale.numel() == N and N > 1 else 0
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        codes = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) if out is None else out
        plane = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_plane else None
    _lib.check_tensor("out", codes, torch.uint8, (N, H, W, 3), device=dev, packed=2, output=True)
    ctx.call("mdvt_nearest_depth_codes", w, h, N, planes.data_ptr(), 4 * planes.stride(1), 4 * planes.stride(0), mw, mh,
             scale.data_ptr() if scale is not None else None, scale_stride, float(max_depth), W, H,
             codes.data_ptr(), codes.stride(1), codes.stride(0), int(bool(bgr)),
             plane.data_ptr() if want_plane else None, 4 * W, 4 * W * H, _lib.stream_arg(dev, s))
    return (codes, plane) if want_plane else codes


def ratio_median(ctx, cv, ref, mask=None, *, want_counts=False, out=None, stream=None):
    """mdvt_ratio_median on float32 CUDA planes cv [N, h_cv, w_cv] and ref [N, h_ref, w_ref] and an optional uint8 CUDA mask
    [N, h_m, w_m] (non-zero = true; rows and frames of the three may be strided) -> the float32 [N] lower medians of the valid ratios
    cv / (ref + 1e-6), 1.0 where none is valid, and with want_counts the int32 [N] counts.  out: the float32 [N] tensor to fill.
    Only enqueues, on `stream`."""
    import torch
    _lib.check_tensor("cv", cv, torch.float32, ndim=3, packed=1, disjoint=True)
    dev = on_context(ctx, "cv", cv)
    N = int(cv.shape[0])
    _lib.check_tensor("ref", ref, torch.float32, (N, None, None), device=dev, packed=1, disjoint=True)
    if N < 1 or min(cv.shape[1:]) < 1 or min(ref.shape[1:]) < 1:
        raise ValueError(f"cv or ref holds no value: shapes {tuple(cv.shape)}, {tuple(ref.shape)}")
    if mask is not None:
        _lib.check_tensor("mask", mask, torch.uint8, (N, None, None), device=dev, packed=1, disjoint=True)
        non_empty("mask", mask, "value")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        median = torch.empty((N,), dtype=torch.float32, device=dev) if out is None else out
        counts = torch.empty((N,), dtype=torch.int32, device=dev) if want_counts else None
    _lib.check_tensor("out", median, torch.float32, (N,), device=dev, contiguous=True, output=True)
    m = (int(mask.shape[2]), int(mask.shape[1]), mask.data_ptr(), mask.stride(1), mask.stride(0)) if mask is not None else (0, 0, None, 0, 0)
    ctx.call("mdvt_ratio_median", N, int(cv.shape[2]), int(cv.shape[1]), cv.data_ptr(), 4 * cv.stride(1), 4 * cv.stride(0),
             int(ref.shape[2]), int(ref.shape[1]), ref.data_ptr(), 4 * ref.stride(1), 4 * ref.stride(0), *m,
             median.data_ptr(), counts.data_ptr() if want_counts else None, _lib.stream_arg(dev, s))
    return (median, counts) if want_counts else median


# ---- include/mdvt_scene.h -----------------------------------------------------------------------------------------------------------

def frame_sums(ctx, frames, prev=None, factor: int = 1, *, bgr: bool = False, stream=None):
    """mdvt_scene_frame_sums on uint8 CUDA frames [n, H, W, 3] with packed pixels (rows and frames may be padded); prev: None or one
    such frame [H, W, 3] on the same device -> the int64 CUDA tensor [pairs, 3] of sum |dH|, |dS|, |dV| (the sums are below 2^63),
    pairs = n - 1 + (prev is not None).  Only enqueues, on `stream` (default: the current stream of the frames' device)."""
    import torch
    dev, n, H, W = frames_on_context(ctx, "frames", frames, "frame")
    if prev is not None:
        _lib.check_tensor("prev", prev, torch.uint8, (H, W, 3), ndim=3, device=dev, packed=2, disjoint=True)
    pairs = n - 1 + (prev is not None)
    if pairs < 1:
        raise ValueError("one frame and no previous frame: no pair to compare")
    factor = int(factor)
    if factor < 1:
        raise ValueError(f"factor must be >= 1, got {factor}")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        sums = torch.empty((pairs, 3), dtype=torch.int64, device=dev)
    ctx.call("mdvt_scene_frame_sums", W, H, n, frames.data_ptr(), frames.stride(1), frames.stride(0), 1 if bgr else 0,
             prev.data_ptr() if prev is not None else None, prev.stride(0) if prev is not None else 0, factor, sums.data_ptr(),
             _lib.stream_arg(dev, s))
    return sums
