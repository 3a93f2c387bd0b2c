"""Device-side mirror of the reference's stereo_dissoclusion_net_infill.py ("sdn", the reference's spelling; movie_2_3D.py's
--infill_engine stereo_dissoclusion_net): the same names and argument meaning, on PyTorch-ROCm tensors through libmdvt_hip.so
(include/mdvt_infill_engines.h).  No CPU fallback.

    sdiss_infill(img, infill_mask, depth_rgb, generate)              sdn:93-123, one eye of a batch of frames
    process_pair(sbs_color, sbs_mask, sbs_depth, generate)           sdn:125-224, on the clip driver's outputs
    python -m metric_depth_video_toolbox_amd.stereo_dissoclusion_net_infill --sbs_color_video X.mkv --sbs_mask_video Y.mkv --sbs_depth_video Z.mkv

The in-painting model is a callable, THE GENERATOR CONTRACT:

    generate(image, infill_mask, depth) -> image

image: uint8 CUDA tensor [N, H, W, 3] (RGB; one eye as rendered), infill_mask: uint8 CUDA tensor [N, H, W, 3] (the finished,
normal-coloured infill mask of that eye), depth: float32 CUDA tensor [N, H, W] (decode_rgb_depth_frame(depth_rgb, 1.0, True), sdn:95:
the eye's coded depth as a fraction of its maximum), all contiguous.  Returns a uint8 CUDA tensor of the shape of `image`, produced
on the current stream.  `--generator pkg.module:callable` names one; the default, `stereo_dissoclusion_net`, calls the net's
`inferance.infer` (sdn:17, 96) frame by frame and needs that checkout, which this project neither ships nor tests against.

Everything behind the model runs on the device in one call per eye and batch (mdvt_model_infill_finish): the 4 x 4 box mean of the
model's image pasted under the mask, the lower side of the holes marked and grown, the 6 x 6 Gaussian under the grown pixels -- the
tail of basic_nomal_infill.normal_infill, on the same listed-pixel stages.  There is no chunk overlap: the reference works frame
by frame.  A mask video that ends early gives black masks (sdn:176-178); a depth video that ends early is a ValueError (the
reference crashes there: sdn:181-186 hands None to cv2.cvtColor).
"""
from __future__ import annotations

import argparse
import importlib
import os

import numpy as np

from . import _lib
from .clip_io import ClipInputs
from .infill_clip import (add_common_flags, callable_from_spec, checked_model_frames, frames4, open_clip, run_batches, run_clips,
                          tuples_from_arguments)


def decode_depth_percent(depth_rgb, out=None):
    """decode_rgb_depth_frame(depth_rgb, 1.0, True) (sdn:95) per frame of uint8 CUDA [N,H,W,3] (rows and frames may be strided: an
    eye's half of side-by-side frames) -> float32 [N,H,W]; out, where given, is that tensor, contiguous, on depth_rgb's GPU."""
    import torch
    frames4(depth_rgb, name="depth_rgb", disjoint=False)      # (one call per frame: any frame stride)
    N, H, W = (int(v) for v in depth_rgb.shape[:3])
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=depth_rgb.device)
    _lib.check_tensor("out", out, torch.float32, (N, H, W), device=depth_rgb, contiguous=True)
    ctx, stream = _lib.shared_context(depth_rgb.device, W, H), _lib.stream_arg(depth_rgb.device)
    for k in range(N):
        ctx.call("mdvt_decode_depth", depth_rgb[k].data_ptr(), depth_rgb.stride(1), out[k].data_ptr(), 4 * W, 1.0, 1.0, stream)
    return out


def model_infill_finish(img, model, infill_mask, out=None):
    """mdvt_model_infill_finish (sdn:100-123 behind the model): uint8 CUDA [N,H,W,3] image, model image and infill mask (rows and
    frames may be strided; out's, where given, without overlap; all on one GPU) -> the finished image; `img` itself is left untouched."""
    import torch
    frames4(img, name="img")
    frames4(model, name="model", shape=tuple(img.shape), device=img)
    frames4(infill_mask, name="infill_mask", shape=tuple(img.shape), device=img)
    N, H, W = (int(v) for v in img.shape[:3])
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=img.device)
    frames4(out, name="out", shape=tuple(img.shape), device=img, output=True)
    _lib.shared_context(img.device).call(
        "mdvt_model_infill_finish", W, H, N, img.data_ptr(), img.stride(1), img.stride(0), model.data_ptr(), model.stride(1), model.stride(0),
        infill_mask.data_ptr(), infill_mask.stride(1), infill_mask.stride(0), out.data_ptr(), out.stride(1), out.stride(0), _lib.stream_arg(img.device))
    return out


def sdiss_infill(img, infill_mask, depth_rgb, generate, out=None):
    """sdn:93-123 for one eye of a batch: uint8 CUDA [N,H,W,3] image, infill mask and coded depth (views of side-by-side frames are
    fine: pixels packed, rows and frames padded at will, not overlapping) -> the infilled image, in `out` where given (the same
    layouts).  The model gets contiguous copies, the library the views themselves.  Unlike the reference, `img` itself is left untouched."""
    frames4(img, name="img")                                  # (everything is held to its contract before the model runs)
    frames4(infill_mask, name="infill_mask", shape=tuple(img.shape), device=img)
    frames4(depth_rgb, name="depth_rgb", shape=tuple(img.shape), device=img, disjoint=False)
    if out is not None:
        frames4(out, name="out", shape=tuple(img.shape), device=img, output=True)
    image, mask = img.contiguous(), infill_mask.contiguous()
    predicted = checked_model_frames(generate(image, mask, decode_depth_percent(depth_rgb)), image)      # sdn:95-96
    return model_infill_finish(img, predicted, infill_mask, out)                              # sdn:100-123


def process_pair(sbs_color_video_path: str, sbs_mask_video_path: str, sbs_depth_video_path: str, generate, max_frames: int = -1, batch: int = 8,
                 device=None, *, video_decoder: str = "host", video_encoder: str = "host"):
    """sdn:125-224.  `.mkv` inputs give `<sbs_color>_infilled.mkv` at the colour video's frame rate, frame dumps (`.npy`, uint8
    [N,H,2W,3]) give `<sbs_color>_infilled.npy`; either is written under its `_tmp_infilled` name and renamed once every frame is in.
    Per batch and eye: the half of colour, mask and coded depth -> sdiss_infill -> that half of the output.  Returns the output path."""
    import torch

    def per_batch(d_color, d_mask, d_depth):
        W = int(d_color.shape[2]) // 2
        d_out = torch.empty_like(d_color)
        for half in (slice(0, W), slice(W, 2 * W)):                # sdn:206, 209: the left eye first
            sdiss_infill(d_color[:, :, half], d_mask[:, :, half], d_depth[:, :, half], generate, out=d_out[:, :, half])
        return d_out
    with ClipInputs() as inp:
        clip = open_clip(inp, sbs_color_video_path, sbs_mask_video_path, [("sbs_depth_video", sbs_depth_video_path, True, "depth video ended early")],
                         max_frames, video_decoder, video_encoder, device)
        run_batches(inp, clip, batch, per_batch)
    return clip.final


class StereoDissoclusionNetGenerator:
    """The default generator: the stereo_dissoclusion_net checkout's `inferance.infer(img, infill_mask, depth_percent)` (sdn:15-17, 96)
    on NumPy arrays, frame by frame.  UNTESTED here (the net is not available to this project)."""

    def __init__(self, checkout: str = "stereo_dissoclusion_net"):
        import sys
        if os.path.abspath(checkout) not in sys.path:
            sys.path.append(os.path.abspath(checkout))
        try:
            self.inferance = importlib.import_module("inferance")
        except ImportError as e:
            raise RuntimeError(f"the stereo_dissoclusion_net generator needs that net's checkout with its inferance module ({e}); "
                               "install it or name another model with --generator pkg.module:callable") from None

    def __call__(self, image, infill_mask, depth):
        import torch
        img, mask, dep = image.cpu().numpy(), infill_mask.cpu().numpy(), depth.cpu().numpy()
        out = np.stack([np.asarray(self.inferance.infer(img[k], mask[k], dep[k])) for k in range(len(img))])
        return torch.from_numpy(np.ascontiguousarray(out.astype(np.uint8))).to(image.device)


def load_generator(spec: str):
    """`stereo_dissoclusion_net` (the default model) or `pkg.module:callable`."""
    return StereoDissoclusionNetGenerator() if spec == "stereo_dissoclusion_net" else callable_from_spec(spec, "stereo_dissoclusion_net")


def triples_from_arguments(sbs_color_video: str, sbs_mask_video: str, sbs_depth_video: str):
    """sdn:238-250: one (sbs_color, sbs_mask, sbs_depth) triple, or -- if the colour argument is a .txt list -- the triples of three
    lists of equal length.  The lists are read and compared before any clip is opened."""
    return tuples_from_arguments([("sbs_color_video", sbs_color_video), ("sbs_mask_video", sbs_mask_video), ("sbs_depth_video", sbs_depth_video)])


def build_parser():
    p = argparse.ArgumentParser(description="Stereo disocclusion net infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--sbs_color_video", type=str, required=True, help="side by side stereo video rendered with point clouds in the masked area (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="side by side stereo video mask, or the matching .txt list")
    p.add_argument("--sbs_depth_video", type=str, required=True, help="side by side stereo depth video, or the matching .txt list")
    p.add_argument("--generator", default="stereo_dissoclusion_net", type=str,
                   help="not a reference flag: the in-painting model, 'stereo_dissoclusion_net' (default) or pkg.module:callable with "
                        "generate(image, infill_mask, depth) -> image on CUDA tensors uint8 [N,H,W,3], uint8 [N,H,W,3] and float32 [N,H,W]")
    return add_common_flags(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = dict(batch=args.batch, video_decoder=args.video_decoder, video_encoder=args.video_encoder)
    return run_clips([("sbs_color_video", args.sbs_color_video), ("sbs_mask_video", args.sbs_mask_video), ("sbs_depth_video", args.sbs_depth_video)],
                     args.max_frames, lambda paths, generate: process_pair(*paths, generate, args.max_frames, **kw), precheck=(True, True, True),
                     load=lambda: load_generator(args.generator))


if __name__ == "__main__":
    import sys
    sys.exit(main())
