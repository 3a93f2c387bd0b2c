"""The device wrappers of the MegaSAM camera-tracking step (tools/sam_track_video.py, tools/megasam_bench.py): the four functions that
hand a tensor's address to the entry points of include/mdvt_megasam.h.  Each takes the clip's context first, refuses a tensor its
docstring does not promise to take before the library sees an address (tests/binding_contract.py holds every one to its record), and
only enqueues on `stream`.  torch is imported inside the functions: importing this module, or a tool, needs none."""
from . import _lib
from .step_clip import non_empty, size_arg, stream_or_current
from .step_device import frames_on_context, on_context


def _sizes(mid_size, crop_size):
    w1, h1 = size_arg(mid_size, "mid_size")
    wc, hc = (w1, h1) if crop_size is None else size_arg(crop_size, "crop_size")
    if wc > w1 or hc > h1:
        raise ValueError(f"crop_size {(wc, hc)} is larger than mid_size {(w1, h1)}")
    return w1, h1, wc, hc


def area_model_frames(ctx, frames, mid_size, crop_size=None, *, bgr=False, stream=None):
    """mdvt_area_model_frames on uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided; B, G, R with bgr) -> the planar uint8
    tensor [N, 3, hc, wc] in R, G, B plane order: cv2.resize(INTER_AREA) to mid_size = (w1, h1), cropped to crop_size = (wc, hc)
    (default: no crop).  Only enqueues, on `stream`."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "frames", frames)
    w1, h1, wc, hc = _sizes(mid_size, crop_size)
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, 3, hc, wc), dtype=torch.uint8, device=dev)
    ctx.call("mdvt_area_model_frames", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w1, h1, wc, hc,
             out.data_ptr(), wc, wc * hc, 3 * wc * hc, _lib.stream_arg(dev, s))
    return out


def tracker_depth(ctx, codes, max_depth, mid_size, crop_size=None, *, bgr=False, stream=None):
    """mdvt_tracker_depth on uint8 CUDA depth frames [N, H, W, 3] (R, G, B; B, G, R with bgr; rows and frames may be strided) ->
    float32 [N, hc, wc]: the depth of R << 24 | B << 16 through torch's nearest-exact resize to mid_size, cropped.  Only enqueues."""
    import torch
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    dev, N, H, W = frames_on_context(ctx, "codes", codes)
    w1, h1, wc, hc = _sizes(mid_size, crop_size)
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, hc, wc), dtype=torch.float32, device=dev)
    ctx.call("mdvt_tracker_depth", W, H, N, codes.data_ptr(), codes.stride(1), codes.stride(0), int(bool(bgr)), float(max_depth), w1, h1, wc, hc,
             out.data_ptr(), 4 * wc, 4 * wc * hc, _lib.stream_arg(dev, s))
    return out


def tracker_mask(ctx, masks, mid_size, crop_size=None, *, bgr=False, stream=None):
    """mdvt_tracker_mask on uint8 CUDA mask frames [N, H, W, 3] (rows and frames may be strided) -> float32 [N, hc, wc]: (255 - grey) /
    255 through torch's bilinear resize to mid_size, cropped.  Only enqueues."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "masks", masks)
    w1, h1, wc, hc = _sizes(mid_size, crop_size)
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, hc, wc), dtype=torch.float32, device=dev)
    ctx.call("mdvt_tracker_mask", W, H, N, masks.data_ptr(), masks.stride(1), masks.stride(0), int(bool(bgr)), w1, h1, wc, hc,
             out.data_ptr(), 4 * wc, 4 * wc * hc, _lib.stream_arg(dev, s))
    return out


def tracker_outputs(ctx, planes, mode, max_value, out_size, *, bgr=False, out=None, stream=None):
    """mdvt_tracker_outputs on float32 CUDA planes [N, h, w] (rows and frames may be strided) -> the uint8 frames [N, H, W, 3] of a
    video at out_size = (W, H).  mode 0: nearest-exact, clip, the 16-bit depth code for max_depth = max_value; mode 1: linear resize,
    clip(x, 0, max_value) / max_value * 255 as three equal bytes.  out: the frames' tensor to fill.  Only enqueues, on `stream`."""
    import torch
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 (depth video) or 1 (grey video), got {mode!r}")
    if not (float(max_value) > 0):
        raise ValueError("max_value must be > 0")
    _lib.check_tensor("planes", planes, torch.float32, ndim=3, packed=1, disjoint=True)
    dev = on_context(ctx, "planes", planes)
    N, h, w = non_empty("planes", planes, "value")
    W, H = size_arg(out_size, "out_size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        frames = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) if out is None else out
    _lib.check_tensor("out", frames, torch.uint8, (N, H, W, 3), device=dev, packed=2, output=True)
    ctx.call("mdvt_tracker_outputs", int(mode), w, h, N, planes.data_ptr(), 4 * planes.stride(1), 4 * planes.stride(0), float(max_value), W, H,
             frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), _lib.stream_arg(dev, s))
    return frames
