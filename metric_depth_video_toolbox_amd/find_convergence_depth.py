"""Device-side mirror of the reference's find_convergence_depth.py (step 4 of movie_2_3D.py, movie_2_3D.py:408-419): per frame of
a depth video the float32 mean of the depths under a mask video's white pixels -- or of all depths -- written as the JSON list that
stereo_rerender.py takes as --convergence_file.  The means are the reference's own float32 numbers bit for bit: NumPy's order of
summation is reproduced by the kernels of csrc/mdvt_convergence.hip (include/mdvt_convergence.h states it).  No CPU fallback.

    convergence_depths(depth_frames, mask_frames)      find_convergence_depth.py:53-80 on device tensors
    find(depth_path, mask_path)                        the whole script: reads the videos, writes <depth_video>_convergence_depths.json
    python -m metric_depth_video_toolbox_amd.find_convergence_depth --depth_video X.mkv [--mask_video M.mkv] [--max_depth 100]
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from . import _lib
from .clip_io import VIDEO_DECODERS, ClipInputs, check_video_decoder, video_parts

SIDECAR_SUFFIX = "_convergence_depths.json"             # fcd:41


def _check_frames(t, name: str):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError(f"{name} must be a uint8 CUDA tensor [N, H, W, 3]")
    if t.shape[0] > 0 and not (t.stride(-1) == 1 and t.stride(-2) == 3):
        raise ValueError(f"{name} must have packed 3-byte pixels (rows and frames may be padded)")
    if t.shape[0] > 0 and (t.stride(1) < 3 * t.shape[2] or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * t.stride(1))):
        raise ValueError(f"{name}: rows or frames overlap (they may be padded, not folded: strides {tuple(t.stride())})")


def convergence_depths(depth_frames, mask_frames=None, max_depth=100, *, bgr: bool = False, counts: bool = False, stream=None):
    """find_convergence_depth.py:53-80 for N frames at once.  depth_frames: uint8 CUDA [N, H, W, 3] (RGB, or BGR with bgr=True; rows and
    frames may be padded); mask_frames: None or uint8 CUDA [M, H, W, 3] with M <= N in the same byte order -- frames from M on use every
    pixel, as the reference does once its mask video has run out.  Returns the float32 CUDA tensor [N] of the means (NaN where a mask
    frame selects nothing); with counts=True also the uint32-valued int32 tensor [N] of the selected pixels.  Only enqueues, on `stream`
    (default: the current stream of the frames' device)."""
    import torch
    _check_frames(depth_frames, "depth_frames")
    N, H, W = (int(v) for v in depth_frames.shape[:3])
    if N < 1:
        raise ValueError("depth_frames holds no frame")
    M = 0
    if mask_frames is not None:
        _check_frames(mask_frames, "mask_frames")
        if mask_frames.device != depth_frames.device:
            raise ValueError("mask_frames and depth_frames are on different devices")
        if tuple(mask_frames.shape[1:3]) != (H, W):
            raise ValueError(f"mask frames are {int(mask_frames.shape[2])}x{int(mask_frames.shape[1])}, depth frames {W}x{H}")
        M = int(mask_frames.shape[0])
        if M > N:
            raise ValueError(f"{M} mask frames for {N} depth frames")
    dev = depth_frames.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        means = torch.empty(N, dtype=torch.float32, device=dev)
        n_sel = torch.empty(N, dtype=torch.int32, device=dev) if counts else None
    order = 1 if bgr else 0
    _lib.shared_context(dev).call(                          # (the render size is irrelevant here too)
        "mdvt_convergence_depths", W, H, depth_frames.data_ptr(), depth_frames.stride(1), depth_frames.stride(0), order,
        mask_frames.data_ptr() if M else None, mask_frames.stride(1) if M else 0, mask_frames.stride(0) if M else 0, order,
        N, M, float(max_depth), means.data_ptr(), n_sel.data_ptr() if counts else None, _lib.stream_arg(dev, s))
    return (means, n_sel) if counts else means


def sidecar_path(depth_path: str) -> str:
    return depth_path + SIDECAR_SUFFIX


def sidecar_text(depths) -> str:
    """The reference's file text (fcd:93-94): json.dumps of the bare list, NaN for a frame whose mask selects nothing."""
    return json.dumps([float(v) for v in depths])


def _check_dump(frames, path: str):
    if frames.ndim != 4 or frames.shape[3] != 3 or frames.dtype != np.uint8:
        raise ValueError(f"{path}: uint8 [N, H, W, 3] expected")
    return frames


def find(depth_path: str, mask_path=None, max_depth=100, *, batch: int = 64, max_frames: int = -1, video_decoder: str = "host"):
    """The reference's script (fcd:15-94): the convergence depth of every frame of the depth video (`.mkv`, or a `.npy` frame dump),
    under the white pixels (gray > 240) of the mask video where one is given.  Writes `<depth_video>_convergence_depths.json` (under a
    temporary name, renamed when complete) and returns the list of Python floats.  A mask video of another size raises ValueError; a
    shorter one prints the reference's "Failed to read mask video frame" (once) and the remaining frames use every pixel.
    video_decoder: "host" (default) or "device" for .mkv files (clip_io.check_video_decoder)."""
    import torch
    with ClipInputs() as inp:
        depth = inp.open(depth_path, "depth video", FileNotFoundError(f"Depth video not found: {depth_path}"))             # fcd:24-25
        mask = None if mask_path is None else \
            inp.open(mask_path, "mask video", FileNotFoundError(f"Mask video not found: {mask_path}"))                     # fcd:29-30
        check_video_decoder(video_decoder, bool(video_parts(depth)))
        if not (float(max_depth) > 0):
            raise ValueError("max_depth must be > 0")
        _check_dump(depth, depth_path)
        if mask is not None and tuple(_check_dump(mask, mask_path).shape[1:3]) != tuple(depth.shape[1:3]):
            raise ValueError(f"Mask video and depth video must have the same dimensions "
                             f"(Mask: {mask.shape[2]}x{mask.shape[1]} vs Depth {depth.shape[2]}x{depth.shape[1]}).")
        n = depth.shape[0] if max_frames < 0 else min(depth.shape[0], max_frames)
        n_mask = min(n, mask.shape[0]) if mask is not None else 0
        batch = max(1, int(batch))
        inp.on_device(torch.device("cuda", torch.cuda.current_device()), video_decoder)
        parts = []
        with torch.cuda.device(inp.dev):
            for a in range(0, n, batch):
                b = min(a + batch, n)
                d_depth = inp.fetch(depth, a, b)
                have = max(0, min(b, n_mask) - a)
                d_mask = inp.fetch(mask, a, a + have) if have else None
                parts.append(convergence_depths(d_depth, d_mask, max_depth))
            means = torch.cat(parts).cpu().numpy() if parts else np.empty(0, np.float32)
        if mask is not None and n_mask < n:
            print("Failed to read mask video frame")                                         # fcd:71
    depths = [float(v) for v in means]                                                       # fcd:78
    out = sidecar_path(depth_path)
    with open(out + ".tmp", "w") as fh:
        fh.write(sidecar_text(depths))
    os.replace(out + ".tmp", out)
    return depths


def build_parser():
    p = argparse.ArgumentParser(description="finds convergence depth in depth video. The depth at which a videos main focus lies. "
                                            "Output can be used to render stereo video with the focus area in convergence.")
    p.add_argument("--depth_video", type=str, required=True, help="depth video to analyse (.mkv, or a .npy frame dump)")
    p.add_argument("--mask_video", type=str, required=False,
                   help="black and white mask video for the main focus area. White where area of interest is.")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses")
    p.add_argument("--batch", default=64, type=int, help="not a reference flag: frames per device call")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="not a reference flag: where the .mkv inputs are FFV1-decoded -- 'host' (default) or 'device' (on the GPU, the "
                        "same bytes; a stream the device does not decode is read on the host) or 'device_all' (as 'device', and Golomb-Rice "
                        "or inter-coded FFV1, FFmpeg's default, is decoded on the GPU as well). Not with .npy inputs")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    depths = find(args.depth_video, args.mask_video, args.max_depth, batch=args.batch, video_decoder=args.video_decoder)
    print(f"Done. Wrote: {sidecar_path(args.depth_video)}  ({len(depths)} frames)")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
