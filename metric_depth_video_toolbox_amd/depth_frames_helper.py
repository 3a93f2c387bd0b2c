"""Device-side mirror of the reference's depth_frames_helper.py codec entry points (same names and
argument meaning), operating on PyTorch-ROCm tensors through the HIP kernels.  No CPU fallback.

  decode_rgb_depth_frame(rgb, max_depth, bit16)     dfh:99-103 (-> dfh:63-75, 13-24)
  encode_depth_frame(depth, max_depth, bgr=True)    dfh:5-11 + dfh:48-61 with bit16=True (sr:930-936)
"""
from __future__ import annotations

from . import _lib


def decode_rgb_depth_frame(rgb, max_depth, bit16=True, depth_scale: float = 1.0, out=None):
    """uint8 device tensor [H,W,3] (RGB order) -> float32 [H,W] metres.  Only the 16-bit format the
    hot path uses is built (bit16 must be True; the reference's 24-bit branch is not on the path).  rgb and out (float32 [H,W] on
    rgb's GPU) must be contiguous: no pitch of theirs is passed on."""
    import torch
    if not bit16:
        raise NotImplementedError("only the bit16 depth format is on the stereo-rerender path")
    _lib.check_tensor("rgb", rgb, torch.uint8, (None, None, 3), contiguous=True)
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=rgb.device)
    _lib.check_tensor("out", out, torch.float32, (H, W), device=rgb, contiguous=True)
    _lib.shared_context(rgb.device, W, H).call("mdvt_decode_depth", rgb.data_ptr(), 3 * W, out.data_ptr(), 4 * W,
                                               float(max_depth), float(depth_scale), _lib.stream_arg(rgb.device))
    return out


def encode_depth_frame(depth, max_depth, bgr: bool = True, out=None):
    """float32 device tensor [H,W] metres -> uint8 [H,W,3] 16-bit depth code, B,G,R order by default
    (what encode_data_as_BGR hands to cv2.VideoWriter) or R,G,B with bgr=False.  depth and out (uint8 [H,W,3] on depth's GPU) must be
    contiguous: no pitch of theirs is passed on."""
    import torch
    _lib.check_tensor("depth", depth, torch.float32, (None, None), contiguous=True)
    H, W = int(depth.shape[0]), int(depth.shape[1])
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=depth.device)
    _lib.check_tensor("out", out, torch.uint8, (H, W, 3), device=depth, contiguous=True)
    _lib.shared_context(depth.device, W, H).call("mdvt_encode_depth", depth.data_ptr(), 4 * W, out.data_ptr(), 3 * W,
                                                 float(max_depth), int(bool(bgr)), _lib.stream_arg(depth.device))
    return out


def swap_rb(frames, out=None):
    """cv2.cvtColor(frame, COLOR_BGR2RGB) / COLOR_RGB2BGR (sr:493, 505, 928, 941) on the device: uint8 CUDA [H,W,3] or
    [N,H,W,3] (rows / images may be strided) -> the same with bytes 0 and 2 of every pixel swapped.  out may be
    `frames` itself (in place)."""
    import torch
    _lib.check_tensor("frames", frames, torch.uint8, (None, None, 3), ndim=(3, 4), packed=2)
    batched = frames.dim() == 4
    N = int(frames.shape[0]) if batched else 1
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    if out is None:
        out = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=frames.device)
    _lib.check_tensor("out", out, torch.uint8, tuple(frames.shape), device=frames, packed=2, output=True)
    _lib.shared_context(frames.device, W, H).call("mdvt_swap_rb", frames.data_ptr(), frames.stride(-3), frames.stride(0) if batched else 0,
                                                  out.data_ptr(), out.stride(-3), out.stride(0) if batched else 0, N,
                                                  _lib.stream_arg(frames.device))
    return out
