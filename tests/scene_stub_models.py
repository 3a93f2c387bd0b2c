"""Stub generators for the movie_2_3D driver's end-to-end test, named on the command line as `scene_stub_models:da3` and
`scene_stub_models:mask` (the tools' --generator contract): cheap functions of the frames, of the kind
tests/test_gpu_da3_clip.py and tests/test_gpu_video_mask_clip.py use.  CALLS counts what ran."""
import numpy as np

CALLS = {"da3": 0, "mask": 0}


def da3(frames, resolution):
    """infer(frames uint8 CUDA [T, H, W, 3], resolution) -> (depth float32 CUDA [T, H, W], extrinsics [T, 3, 4], intrinsics [T, 3, 3])."""
    import torch
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3
    CALLS["da3"] += 1
    T, H, W = (int(v) for v in frames.shape[:3])
    depth = frames[..., 0].float() / 16.0 + 2.0 + torch.arange(W, device=frames.device, dtype=torch.float32) / 8.0
    ext = np.tile(np.eye(4)[:3][None], (T, 1, 1))
    ext[:, 0, 3] = -0.01 * np.arange(T)
    intr = np.tile(np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]])[None], (T, 1, 1))
    return depth.contiguous(), ext, intr


def mask(x):
    """infer(x float32 CUDA [n, 3, S, S]) -> the prediction float32 CUDA [n, S, S]."""
    assert x.is_cuda and x.dim() == 4 and x.shape[1] == 3
    CALLS["mask"] += 1
    return (x[:, 0] - x[:, 2]).contiguous()
