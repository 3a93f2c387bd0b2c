"""Device-side mirror of the reference's infill_common.mark_lower_side (infill_common.py:4-49), same name
and argument meaning, on PyTorch-ROCm tensors through the HIP kernel.  No CPU fallback."""
from __future__ import annotations

from . import _lib


def mark_lower_side(normals_img, max_steps=30, out=None):
    """normals_img: uint8 CUDA tensor [H,W,3] (the normal-coloured infill mask; black = not a hole).
    Returns a uint8 [H,W,3] tensor that is (0,0,255) where a hole pixel's march along its encoded XY
    direction is about to leave the hole ("the lower side"), 0 elsewhere.  normals_img may have any layout (a strided one is
    copied); out, where given, must be a contiguous uint8 [H,W,3] tensor on the same GPU."""
    import torch
    _lib.check_tensor("normals_img", normals_img, torch.uint8, (None, None, 3))
    img = normals_img.contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    if out is None:
        out = torch.empty_like(img)
    _lib.check_tensor("out", out, torch.uint8, (H, W, 3), device=img, contiguous=True)
    _lib.shared_context(img.device, W, H).call("mdvt_mark_lower_side", img.data_ptr(), 3 * W, out.data_ptr(), 3 * W, int(max_steps),
                                               _lib.stream_arg(img.device))
    return out
