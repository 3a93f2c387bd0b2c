"""The device wrappers of the InSpatio-World infill step's alignment (tools/inspatio_world_infill.py, tools/inspatio_bench.py): the
five functions that hand tensors' addresses to mdvt_inspatio_prepare_eye, mdvt_inspatio_model_frames, mdvt_masked_shift_grid,
mdvt_flow_warp and mdvt_inspatio_composite_eye (include/mdvt_inspatio.h).  Each takes the clip's context first, refuses a tensor its
docstring does not promise to take before the library sees an address (tests/binding_contract.py holds every one to its record), and
only enqueues on `stream`.  torch is imported inside the functions: importing this module, or a tool, needs none.  model_frames here
is this step's u8 resize, not step_device.model_frames."""
from . import _lib
from .step_clip import size_arg, stream_or_current
from .step_device import frames_on_context


def _eye(eye):
    if eye not in (0, 1):
        raise ValueError(f"eye must be 0 or 1, got {eye!r}")
    return int(eye)


def masked_shift_grid(ctx, render, infilled, valid, *, path=0, stream=None):
    """mdvt_masked_shift_grid on one eye's uint8 CUDA frames: render and infilled [N, H, W, 3], valid [N, H, W] (non-zero = valid;
    rows and frames may be strided) -> (shift float64 [N, 4, 4, 2] (dy, dx), status uint8 [N, 4, 4], round_error float64 [1]: the
    largest distance from an integer the transform path rounded, 0 on the direct path).  path: 0 as mdvt_masked_shift_path says, 1
    direct, 2 transform.  Only enqueues, on `stream`: nothing is read back."""
    import torch
    if path not in (_lib.SHIFT_PATH_AUTO, _lib.SHIFT_PATH_DIRECT, _lib.SHIFT_PATH_TRANSFORM):
        raise ValueError(f"path must be 0 (auto), 1 (direct) or 2 (transform), got {path!r}")
    dev, N, H, W = frames_on_context(ctx, "render", render)
    _lib.check_tensor("infilled", infilled, torch.uint8, (N, H, W, 3), ndim=4, device=dev, packed=2, disjoint=True)
    _lib.check_tensor("valid", valid, torch.uint8, (N, H, W), ndim=3, device=dev, packed=1, disjoint=True)
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        shift = torch.empty((N, 4, 4, 2), dtype=torch.float64, device=dev)
        status = torch.empty((N, 4, 4), dtype=torch.uint8, device=dev)
        err = torch.empty((1,), dtype=torch.float64, device=dev)
    ctx.call("mdvt_masked_shift_grid", W, H, N, render.data_ptr(), render.stride(1), render.stride(0),
             infilled.data_ptr(), infilled.stride(1), infilled.stride(0), valid.data_ptr(), valid.stride(1), valid.stride(0),
             int(path), shift.data_ptr(), status.data_ptr(), err.data_ptr(), _lib.stream_arg(dev, s))
    return shift, status, err


def flow_warp(ctx, grids, has_grid, infilled, *, out=None, stream=None):
    """mdvt_flow_warp: grids float32 CUDA [N, 4, 4, 2] (dx, dy; contiguous), has_grid uint8 CUDA [N] (contiguous) and the infilled
    frames uint8 CUDA [N, H, W, 3] (rows and frames may be strided) -> the aligned frames [N, H, W, 3]; a frame without a grid is
    copied.  out: the tensor to fill (it must not overlap infilled).  Only enqueues, on `stream`."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "infilled", infilled)
    _lib.check_tensor("grids", grids, torch.float32, (N, 4, 4, 2), ndim=4, device=dev, contiguous=True)
    _lib.check_tensor("has_grid", has_grid, torch.uint8, (N,), ndim=1, device=dev, contiguous=True)
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        frames = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) if out is None else out
    _lib.check_tensor("out", frames, torch.uint8, (N, H, W, 3), device=dev, packed=2, output=True)
    ctx.call("mdvt_flow_warp", W, H, N, grids.data_ptr(), has_grid.data_ptr(), infilled.data_ptr(), infilled.stride(1), infilled.stride(0),
             frames.data_ptr(), frames.stride(1), frames.stride(0), _lib.stream_arg(dev, s))
    return frames


def prepare_eye(ctx, sbs_color, sbs_mask, eye, model_size, *, stream=None):
    """mdvt_inspatio_prepare_eye on uint8 CUDA side-by-side frames [N, H, 2W, 3] (rows and frames may be strided) -> (valid [N, H, W],
    render [N, H, W, 3] with the holes black, model_valid [N, mh, mw], model_render [N, mh, mw, 3], hole_counts int32 [N] on the
    device); eye 0 is the left half, 1 the right; model_size = (mw, mh).  Only enqueues, on `stream`."""
    import torch
    eye = _eye(eye)
    dev, N, H, W2 = frames_on_context(ctx, "sbs_color", sbs_color)
    if W2 % 2:
        raise ValueError(f"sbs_color must have an even width, got {W2}")
    _lib.check_tensor("sbs_mask", sbs_mask, torch.uint8, (N, H, W2, 3), ndim=4, device=dev, packed=2, disjoint=True)
    W = W2 // 2
    mw, mh = size_arg(model_size, "model_size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        valid = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        render = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        m_valid = torch.empty((N, mh, mw), dtype=torch.uint8, device=dev)
        m_render = torch.empty((N, mh, mw, 3), dtype=torch.uint8, device=dev)
        holes = torch.empty((N,), dtype=torch.int32, device=dev)
    ctx.call("mdvt_inspatio_prepare_eye", W, H, N, eye, sbs_color.data_ptr(), sbs_color.stride(1), sbs_color.stride(0),
             sbs_mask.data_ptr(), sbs_mask.stride(1), sbs_mask.stride(0), mw, mh, valid.data_ptr(), W, W * H, render.data_ptr(), 3 * W, 3 * W * H,
             m_valid.data_ptr(), mw, mw * mh, m_render.data_ptr(), 3 * mw, 3 * mw * mh, holes.data_ptr(), _lib.stream_arg(dev, s))
    return valid, render, m_valid, m_render, holes


def model_frames(ctx, frames, size, *, stream=None):
    """mdvt_inspatio_model_frames: uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided) through the u8 resize to size =
    (w, h) -> [N, h, w, 3].  Only enqueues, on `stream`."""
    import torch
    dev, N, H, W = frames_on_context(ctx, "frames", frames)
    w, h = size_arg(size, "size")
    s = stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, h, w, 3), dtype=torch.uint8, device=dev)
    ctx.call("mdvt_inspatio_model_frames", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), w, h, out.data_ptr(), 3 * w, 3 * w * h,
             _lib.stream_arg(dev, s))
    return out


def composite_eye(ctx, aligned, sbs_color, sbs_mask, eye, pasted, blended=None, *, stream=None):
    """mdvt_inspatio_composite_eye: the aligned frames uint8 CUDA [N, H, W, 3] pasted under the holes of that eye's half of the
    side-by-side frames [N, H, 2W, 3] into `pasted`, and, where `blended` is given, blended along the holes' lower side into it (both
    uint8 CUDA [N, H, 2W, 3]; the eye's half is written).  Rows and frames may be strided.  Only enqueues, on `stream`."""
    import torch
    eye = _eye(eye)
    dev, N, H, W = frames_on_context(ctx, "aligned", aligned)
    _lib.check_tensor("sbs_color", sbs_color, torch.uint8, (N, H, 2 * W, 3), ndim=4, device=dev, packed=2, disjoint=True)
    _lib.check_tensor("sbs_mask", sbs_mask, torch.uint8, (N, H, 2 * W, 3), ndim=4, device=dev, packed=2, disjoint=True)
    _lib.check_tensor("pasted", pasted, torch.uint8, (N, H, 2 * W, 3), ndim=4, device=dev, packed=2, output=True)
    if blended is not None:
        _lib.check_tensor("blended", blended, torch.uint8, (N, H, 2 * W, 3), ndim=4, device=dev, packed=2, output=True)
    s = stream_or_current(dev, stream)
    b = (None, 0, 0) if blended is None else (blended.data_ptr(), blended.stride(1), blended.stride(0))
    ctx.call("mdvt_inspatio_composite_eye", W, H, N, eye, aligned.data_ptr(), aligned.stride(1), aligned.stride(0),
             sbs_color.data_ptr(), sbs_color.stride(1), sbs_color.stride(0), sbs_mask.data_ptr(), sbs_mask.stride(1), sbs_mask.stride(0),
             pasted.data_ptr(), pasted.stride(1), pasted.stride(0), *b, _lib.stream_arg(dev, s))
    return pasted, blended
