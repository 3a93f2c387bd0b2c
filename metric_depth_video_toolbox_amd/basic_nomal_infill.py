"""Device-side mirror of the reference's basic_nomal_infill.py (movie_2_3D.py's infill step after stereo_rerender): the
same names and argument meaning, on PyTorch-ROCm tensors through libmdvt_hip.so.  No CPU fallback.

    normal_infill(img, infill_mask)            basic_nomal_infill.py:87-119, one eye
    process_pair(sbs_color, sbs_mask)          basic_nomal_infill.py:124-236, on the clip driver's outputs (clip.py's formats)
    python -m metric_depth_video_toolbox_amd.basic_nomal_infill --sbs_color_video X.mkv --sbs_mask_video Y.mkv

The reference reads and writes FFV1 videos through OpenCV (bni:129-145).  So does this module when the inputs are the `.mkv`
files the clip driver writes (`<depth>_stereo.mkv`, `<depth>_stereo.mkv_infillmask.mkv`): the output is
`<sbs_color>_infilled.mkv` (the reference appends `_infilled.mkv` to the colour video's full name, bni:141), optionally decoded
and encoded on the GPU (--video_decoder / --video_encoder device).  With the `.npy` dumps the clip driver writes for `.npy`
inputs (uint8 [N, H, 2W, 3], RGB order) the output is `<sbs_color>_infilled.npy`.  Either is written under its `_tmp_infilled`
name and renamed once every frame is in (clip_io.verify_and_move, dfh:163-179).
"""
from __future__ import annotations

import argparse

from . import _lib
from .clip_io import ClipInputs
from .infill_clip import add_common_flags, open_clip, run_batches, run_clips, tuples_from_arguments


def normal_infill(img, infill_mask, out=None):
    """basic_nomal_infill.normal_infill (basic_nomal_infill.py:87-119).  img, infill_mask: uint8 CUDA tensors [H,W,3] or
    [N,H,W,3] (RGB; rows and images may be strided, e.g. one half of a side-by-side frame).  Returns the image with its
    holes filled.  Unlike the reference, `img` itself is left untouched (the reference blackens and refills it in place
    and returns a new array; its caller only uses the returned one, basic_nomal_infill.py:186)."""
    import torch
    _lib.check_tensor("img", img, torch.uint8, (None, None, 3), ndim=(3, 4), packed=2)
    _lib.check_tensor("infill_mask", infill_mask, torch.uint8, tuple(img.shape), device=img, packed=2)
    batched = img.dim() == 4
    N = int(img.shape[0]) if batched else 1
    H, W = int(img.shape[-3]), int(img.shape[-2])
    if out is None:
        out = torch.empty(tuple(img.shape), dtype=torch.uint8, device=img.device)
    _lib.check_tensor("out", out, torch.uint8, tuple(img.shape), device=img, packed=2, output=True)
    stride = (lambda t: t.stride(0) if batched else 0)
    _lib.shared_context(img.device, W, H).call("mdvt_normal_infill", img.data_ptr(), img.stride(-3), stride(img),
                                               infill_mask.data_ptr(), infill_mask.stride(-3), stride(infill_mask),
                                               out.data_ptr(), out.stride(-3), stride(out), N, _lib.stream_arg(img.device))
    return out


def normal_infill_sbs(sbs, sbs_mask, out=None):
    """Both eyes of side-by-side frames (basic_nomal_infill.py:172-228): uint8 CUDA [N,H,2W,3] (or [H,2W,3]) -> the same
    layout with both halves infilled."""
    import torch
    if out is None:
        out = torch.empty(tuple(sbs.shape), dtype=torch.uint8, device=sbs.device)
    W = int(sbs.shape[-2]) // 2
    for half in (slice(0, W), slice(W, 2 * W)):
        normal_infill(sbs[..., half, :], sbs_mask[..., half, :], out=out[..., half, :])
    return out


def process_pair(sbs_color_video_path: str, sbs_mask_video_path: str, max_frames: int = -1, batch: int = 8, device=None, *,
                 video_decoder: str = "host", video_encoder: str = "host"):
    """basic_nomal_infill.process_pair (basic_nomal_infill.py:124-236).  `.mkv` inputs (the reference's format: `<x>_stereo.mkv`
    and `<x>_stereo.mkv_infillmask.mkv`, bni:129-145) give `<sbs_color>_infilled.mkv` at the colour video's frame rate, frame
    dumps give `<sbs_color>_infilled.npy`; either is written under its `_tmp_infilled` name and renamed once every frame is in.
    A mask clip shorter than the colour clip means "no holes" for the remaining frames (basic_nomal_infill.py:165-167).
    video_decoder / video_encoder: "host" (default) or "device" for .mkv files (the same bytes; clip_io.check_video_decoder /
    check_video_encoder refuse "device" for frame dumps).  Returns the output path."""
    with ClipInputs() as inp:
        clip = open_clip(inp, sbs_color_video_path, sbs_mask_video_path, [], max_frames, video_decoder, video_encoder, device, allow_empty=True,
                         zero_frames="max_frames = 0: the reference still processes one frame (bni:226-228); ask for -1 (all) or a positive count")
        run_batches(inp, clip, batch, normal_infill_sbs)
    return clip.final


def pairs_from_arguments(sbs_color_video: str, sbs_mask_video: str):
    """bni:246-260: one pair, or -- if the colour argument is a .txt list -- the pairs of two lists of equal length."""
    return tuples_from_arguments([("sbs_color_video", sbs_color_video), ("sbs_mask_video", sbs_mask_video)])


def build_parser():
    p = argparse.ArgumentParser(description="Normal infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--sbs_color_video", type=str, required=True, help="side by side stereo video (.mkv, or a .npy frame dump) rendered with point clouds in the masked area, or a .txt list of them")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="side by side infill mask video (.mkv, or a .npy frame dump), or the matching .txt list")
    return add_common_flags(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = dict(batch=args.batch, video_decoder=args.video_decoder, video_encoder=args.video_encoder)
    return run_clips([("sbs_color_video", args.sbs_color_video), ("sbs_mask_video", args.sbs_mask_video)], args.max_frames,
                     lambda paths, _: process_pair(*paths, args.max_frames, **kw))


if __name__ == "__main__":
    import sys
    sys.exit(main())
