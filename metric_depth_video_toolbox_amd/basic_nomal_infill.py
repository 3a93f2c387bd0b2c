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

import numpy as np

from . import _lib
from .clip_io import VIDEO_DECODERS, ClipInputs, ClipOutput, check_video_decoder, check_video_encoder, video_parts


def _packed(t):
    return t.stride(-1) == 1 and t.stride(-2) == 3


def normal_infill(img, infill_mask, out=None):
    """basic_nomal_infill.normal_infill (basic_nomal_infill.py:87-119).  img, infill_mask: uint8 CUDA tensors [H,W,3] or
    [N,H,W,3] (RGB; rows and images may be strided, e.g. one half of a side-by-side frame).  Returns the image with its
    holes filled.  Unlike the reference, `img` itself is left untouched (the reference blackens and refills it in place
    and returns a new array; its caller only uses the returned one, basic_nomal_infill.py:186)."""
    import torch
    for t in (img, infill_mask):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() in (3, 4) and t.shape[-1] == 3 and _packed(t), \
            "uint8 CUDA [H,W,3] or [N,H,W,3] with packed RGB pixels"
    assert img.shape == infill_mask.shape
    batched = img.dim() == 4
    N = int(img.shape[0]) if batched else 1
    H, W = int(img.shape[-3]), int(img.shape[-2])
    if out is None:
        out = torch.empty(tuple(img.shape), dtype=torch.uint8, device=img.device)
    assert out.shape == img.shape and out.is_cuda and out.dtype == torch.uint8 and _packed(out)
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
    import torch
    with ClipInputs() as inp:
        # (a clip rendered by several ranks exists as per-rank segments + index: run_output reads either form)
        color = inp.open(sbs_color_video_path, "sbs_color_video", Exception(f"input sbs_color_video does not exist: {sbs_color_video_path}"), True)
        mask = inp.open(sbs_mask_video_path, "sbs_mask_video", Exception(f"input sbs_mask_video does not exist: {sbs_mask_video_path}"), True)
        video = bool(video_parts(color))
        check_video_decoder(video_decoder, video)
        check_video_encoder(video_encoder, video)
        assert color.ndim == 4 and color.shape[-1] == 3 and color.dtype == np.uint8, "uint8 [N, H, 2W, 3] expected"
        assert color.shape[1:] == mask.shape[1:], "mask and color video not same resolution"
        if color.shape[2] % 2:
            raise ValueError(f"side-by-side frames need an even width, got {color.shape[2]}")     # (the reference gives the right eye the odd column: bni:180-181)
        if max_frames == 0:
            raise ValueError("max_frames = 0: the reference still processes one frame (bni:226-228); ask for -1 (all) or a positive count")
        n = color.shape[0] if max_frames == -1 else min(color.shape[0], max_frames)
        batch = max(1, int(batch))
        ext = ".mkv" if video else ".npy"
        tmp, final = sbs_color_video_path + "_tmp_infilled" + ext, sbs_color_video_path + "_infilled" + ext      # bni:140-141
        fps = (video_parts(color)[0][0].fps or 30.0) if video else None                      # bni:134: the colour video's frame rate
        inp.on_device(torch.device("cuda", torch.cuda.current_device() if device is None else device), video_decoder, video_encoder)
        with ClipOutput(tmp, final, n, color.shape[1:], fps, video_encoder, inp.ctx) as out, torch.cuda.device(inp.dev):
            for a in range(0, n, batch):
                b = min(a + batch, n)
                d_color = inp.fetch(color, a, b)
                have = max(0, min(b, mask.shape[0]) - a)
                if have == b - a:
                    d_mask = inp.fetch(mask, a, b)
                else:
                    d_mask = torch.zeros((b - a,) + tuple(color.shape[1:]), dtype=torch.uint8, device=inp.dev)
                    if have:
                        d_mask[:have] = inp.fetch(mask, a, a + have)
                out.store(normal_infill_sbs(d_color, d_mask), a)
    return final


def _is_txt(path) -> bool:
    return isinstance(path, str) and path.lower().endswith(".txt")                      # bni:29-30


def _read_list_file(path: str):
    """Stripped lines of a list file, blank lines and lines starting with '#' ignored (bni:32-43)."""
    with open(path, "r", encoding="utf-8") as f:
        return [ln.strip() for ln in f if ln.strip() and not ln.strip().startswith("#")]


def pairs_from_arguments(sbs_color_video: str, sbs_mask_video: str):
    """bni:246-260: one pair, or -- if the colour argument is a .txt list -- the pairs of two lists of equal length."""
    if not _is_txt(sbs_color_video):
        return [(sbs_color_video, sbs_mask_video)]
    if not _is_txt(sbs_mask_video):
        raise ValueError("If --sbs_color_video is a .txt file, then --sbs_mask_video must also be a .txt file.")
    colors, masks = _read_list_file(sbs_color_video), _read_list_file(sbs_mask_video)
    if len(colors) != len(masks):
        raise ValueError(f"List length mismatch: {sbs_color_video} has {len(colors)} entries, {sbs_mask_video} has {len(masks)} entries.")
    return list(zip(colors, masks))


def build_parser():
    p = argparse.ArgumentParser(description="Normal infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--sbs_color_video", type=str, required=True, help="side by side stereo video (.mkv, or a .npy frame dump) rendered with point clouds in the masked area, or a .txt list of them")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="side by side infill mask video (.mkv, or a .npy frame dump), or the matching .txt list")
    p.add_argument("--max_frames", default=-1, type=int, help="quit after max_frames nr of frames", required=False)
    p.add_argument("--batch", default=8, type=int, help="not a reference flag: frames per device batch")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="not a reference flag: where the .mkv inputs are FFV1-decoded -- 'host' (default) or 'device' (on the GPU, the "
                        "same bytes; only the compressed packets are copied to the device; a stream the device does not decode is "
                        "read on the host) or 'device_all' (as 'device', and Golomb-Rice or inter-coded FFV1, FFmpeg's default, is "
                        "decoded on the GPU as well). Not with .npy inputs")
    p.add_argument("--video_encoder", choices=("host", "device"), default="host",
                   help="not a reference flag: where the .mkv output is FFV1-encoded -- 'host' (default) or 'device' (on the GPU, the "
                        "same bytes). Not with .npy inputs")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = dict(batch=args.batch, video_decoder=args.video_decoder, video_encoder=args.video_encoder)
    pairs = pairs_from_arguments(args.sbs_color_video, args.sbs_mask_video)
    if _is_txt(args.sbs_color_video):
        # (the reference runs two clips at a time with the GPU sections serialised, bni:262-274; here a clip is I/O and one
        #  launch set per batch, so the clips simply follow each other)
        print(f"Batch mode: {len(pairs)} pairs")
        for c_path, m_path in pairs:
            try:
                print("Done. Wrote:", process_pair(c_path, m_path, args.max_frames, **kw))
            except Exception as e:                                    # bni:270-274: surface the error, keep the other clips going
                print(f"[ERROR] A clip failed: {e}")
        return 0
    print("Done. Wrote:", process_pair(*pairs[0], args.max_frames, **kw))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
