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
from .basic_nomal_infill import _is_txt, _read_list_file
from .clip_io import VIDEO_DECODERS, ClipInputs, ClipOutput, check_video_decoder, check_video_encoder, video_parts
from .stereo_crafter_infill import _frames4, callable_from_spec


def decode_depth_percent(depth_rgb, out=None):
    """decode_rgb_depth_frame(depth_rgb, 1.0, True) (sdn:95) per frame of uint8 CUDA [N,H,W,3] (rows and frames may be strided: an
    eye's half of side-by-side frames) -> float32 [N,H,W]."""
    import torch
    _frames4(depth_rgb)
    N, H, W = (int(v) for v in depth_rgb.shape[:3])
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.float32, device=depth_rgb.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (N, H, W)
    ctx, stream = _lib.shared_context(depth_rgb.device, W, H), _lib.stream_arg(depth_rgb.device)
    for k in range(N):
        ctx.call("mdvt_decode_depth", depth_rgb[k].data_ptr(), depth_rgb.stride(1), out[k].data_ptr(), 4 * W, 1.0, 1.0, stream)
    return out


def model_infill_finish(img, model, infill_mask, out=None):
    """mdvt_model_infill_finish (sdn:100-123 behind the model): uint8 CUDA [N,H,W,3] image, model image and infill mask (rows and
    frames may be strided) -> the finished image; `img` itself is left untouched."""
    import torch
    for t in (img, model, infill_mask):
        _frames4(t)
    assert img.shape == model.shape == infill_mask.shape
    N, H, W = (int(v) for v in img.shape[:3])
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=img.device)
    _frames4(out)
    assert out.shape == img.shape
    _lib.shared_context(img.device).call(
        "mdvt_model_infill_finish", W, H, N, img.data_ptr(), img.stride(1), img.stride(0), model.data_ptr(), model.stride(1), model.stride(0),
        infill_mask.data_ptr(), infill_mask.stride(1), infill_mask.stride(0), out.data_ptr(), out.stride(1), out.stride(0), _lib.stream_arg(img.device))
    return out


def sdiss_infill(img, infill_mask, depth_rgb, generate, out=None):
    """sdn:93-123 for one eye of a batch: uint8 CUDA [N,H,W,3] image, infill mask and coded depth (views of side-by-side frames are
    fine) -> the infilled image.  Unlike the reference, `img` itself is left untouched."""
    import torch
    image, mask = img.contiguous(), infill_mask.contiguous()
    predicted = generate(image, mask, decode_depth_percent(depth_rgb))                        # sdn:95-96
    if not (torch.is_tensor(predicted) and predicted.is_cuda and predicted.dtype == torch.uint8 and predicted.shape == image.shape):
        raise TypeError(f"the generator must return a uint8 CUDA tensor of shape {tuple(image.shape)}")
    return model_infill_finish(img, predicted.contiguous(), infill_mask, out)                 # sdn:100-123


def process_pair(sbs_color_video_path: str, sbs_mask_video_path: str, sbs_depth_video_path: str, generate, max_frames: int = -1, batch: int = 8,
                 device=None, *, video_decoder: str = "host", video_encoder: str = "host"):
    """sdn:125-224.  `.mkv` inputs give `<sbs_color>_infilled.mkv` at the colour video's frame rate, frame dumps (`.npy`, uint8
    [N,H,2W,3]) give `<sbs_color>_infilled.npy`; either is written under its `_tmp_infilled` name and renamed once every frame is in.
    Per batch and eye: the half of colour, mask and coded depth -> sdiss_infill -> that half of the output.  Returns the output path."""
    import torch
    with ClipInputs() as inp:
        color = inp.open(sbs_color_video_path, "sbs_color_video", Exception(f"input sbs_color_video does not exist: {sbs_color_video_path}"), True)
        mask = inp.open(sbs_mask_video_path, "sbs_mask_video", Exception(f"input sbs_mask_video does not exist: {sbs_mask_video_path}"), True)
        depth = inp.open(sbs_depth_video_path, "sbs_depth_video", Exception(f"input sbs_depth_video does not exist: {sbs_depth_video_path}"), True)
        video = bool(video_parts(color))
        check_video_decoder(video_decoder, video)
        check_video_encoder(video_encoder, video)
        assert color.ndim == 4 and color.shape[-1] == 3 and color.dtype == np.uint8, "uint8 [N, H, 2W, 3] expected"
        assert color.shape[1:] == mask.shape[1:] == depth.shape[1:], "mask and color video not same resolution"      # sdn:147
        if color.shape[2] % 2:
            raise ValueError(f"side-by-side frames need an even width, got {color.shape[2]}")
        if max_frames == 0:
            raise ValueError("max_frames = 0: ask for -1 (all) or a positive count")
        n = color.shape[0] if max_frames == -1 else min(color.shape[0], max_frames)
        if n < 1:
            raise ValueError(f"{sbs_color_video_path} has no frames")
        if depth.shape[0] < n:
            raise ValueError(f"depth video ended early: {sbs_depth_video_path} has {depth.shape[0]} frames, {n} are needed")
        batch = max(1, int(batch))
        ext = ".mkv" if video else ".npy"
        tmp, final = sbs_color_video_path + "_tmp_infilled" + ext, sbs_color_video_path + "_infilled" + ext      # sdn:151-152
        fps = (video_parts(color)[0][0].fps or 30.0) if video else None
        W = int(color.shape[2]) // 2
        inp.on_device(torch.device("cuda", torch.cuda.current_device() if device is None else device), video_decoder, video_encoder)
        with ClipOutput(tmp, final, n, color.shape[1:], fps, video_encoder, inp.ctx) as out, torch.cuda.device(inp.dev):
            for a in range(0, n, batch):
                b = min(a + batch, n)
                d_color, d_depth = inp.fetch(color, a, b), inp.fetch(depth, a, b)
                have = max(0, min(b, mask.shape[0]) - a)
                if have == b - a:
                    d_mask = inp.fetch(mask, a, b)
                else:                                              # sdn:176-178
                    d_mask = torch.zeros((b - a,) + tuple(color.shape[1:]), dtype=torch.uint8, device=inp.dev)
                    if have:
                        d_mask[:have] = inp.fetch(mask, a, a + have)
                d_out = torch.empty_like(d_color)
                for half in (slice(0, W), slice(W, 2 * W)):        # sdn:206, 209: the left eye first
                    sdiss_infill(d_color[:, :, half], d_mask[:, :, half], d_depth[:, :, half], generate, out=d_out[:, :, half])
                out.store(d_out, a)
    return final


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
    if not _is_txt(sbs_color_video):
        return [(sbs_color_video, sbs_mask_video, sbs_depth_video)]
    if not _is_txt(sbs_mask_video) or not _is_txt(sbs_depth_video):
        raise ValueError("If --sbs_color_video is a .txt file, then --sbs_mask_video and --sbs_depth_video must also be .txt files.")
    colors, masks, depths = _read_list_file(sbs_color_video), _read_list_file(sbs_mask_video), _read_list_file(sbs_depth_video)
    if len(colors) != len(masks) or len(colors) != len(depths):
        raise ValueError(f"List length mismatch: {sbs_color_video} has {len(colors)} entries, {sbs_mask_video} has {len(masks)} entries, "
                         f"{sbs_depth_video} has {len(depths)} entries.")
    return list(zip(colors, masks, depths))


def build_parser():
    p = argparse.ArgumentParser(description="Stereo disocclusion net infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--sbs_color_video", type=str, required=True, help="side by side stereo video rendered with point clouds in the masked area (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="side by side stereo video mask, or the matching .txt list")
    p.add_argument("--sbs_depth_video", type=str, required=True, help="side by side stereo depth video, or the matching .txt list")
    p.add_argument("--max_frames", default=-1, type=int, help="quit after max_frames nr of frames", required=False)
    p.add_argument("--generator", default="stereo_dissoclusion_net", type=str,
                   help="not a reference flag: the in-painting model, 'stereo_dissoclusion_net' (default) or pkg.module:callable with "
                        "generate(image, infill_mask, depth) -> image on CUDA tensors uint8 [N,H,W,3], uint8 [N,H,W,3] and float32 [N,H,W]")
    p.add_argument("--batch", default=8, type=int, help="not a reference flag: frames per device batch")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="not a reference flag: where the .mkv inputs are FFV1-decoded -- 'host' (default), 'device' (on the GPU, the same bytes) "
                        "or 'device_all' (as 'device', and Golomb-Rice or inter-coded FFV1, FFmpeg's default, as well). Not with .npy inputs")
    p.add_argument("--video_encoder", choices=("host", "device"), default="host",
                   help="not a reference flag: where the .mkv output is FFV1-encoded -- 'host' (default) or 'device' (on the GPU, the same bytes). Not with .npy inputs")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.max_frames == 0:
        raise SystemExit("--max_frames 0: ask for -1 (all) or a positive count")
    triples = triples_from_arguments(args.sbs_color_video, args.sbs_mask_video, args.sbs_depth_video)
    listed = _is_txt(args.sbs_color_video)
    for paths in triples:
        for what, path in zip(("sbs_color_video", "sbs_mask_video", "sbs_depth_video"), paths):
            if not listed and not (os.path.isfile(path) or os.path.isfile(path + ".index.json")):
                raise SystemExit(f"input {what} does not exist: {path}")
    try:
        generate = load_generator(args.generator)
    except (RuntimeError, ValueError, ImportError) as e:
        raise SystemExit(str(e))
    kw = dict(batch=args.batch, video_decoder=args.video_decoder, video_encoder=args.video_encoder)
    if listed:
        # (the reference runs two clips at a time, sdn:252-263; here the clips follow each other)
        print(f"Batch mode: {len(triples)} pairs")
        for c_path, m_path, d_path in triples:
            try:
                print("Done. Wrote:", process_pair(c_path, m_path, d_path, generate, args.max_frames, **kw))
            except Exception as e:                                # sdn:261-263: surface the error, keep the other clips going
                print(f"[ERROR] A clip failed: {e}")
        return 0
    print("Done. Wrote:", process_pair(*triples[0], generate, args.max_frames, **kw))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
