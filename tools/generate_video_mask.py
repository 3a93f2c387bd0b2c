#!/usr/bin/env python3
"""The reference's generate_video_mask.py (gvm:) around its model, on the device: step 3 of movie_2_3D.py, which writes the black and
white video of the main subject that find_convergence_depth --mask_video and stereo_rerender --convergence_mask_video read.

    python tools/generate_video_mask.py --color_video x.mkv|list.txt [--max_frames N --batch_size 8 --model_size 320
           --video_decoder host|device|device_all --video_encoder host|device] [--generator pkg.module:callable]

writes x.mkv_mask.mkv (tmp x.mkv_tmp_mask.mkv, renamed when its frame count is right).  A .txt list runs each entry; a .npy frame dump
gives a .npy mask.  INTEGRATION.md states the generator's contract.

The parser, the file names and U2-Net's constants are host logic in metric_depth_video_toolbox_amd/video_mask.py.  Here is what touches
the device, per batch: the decoded frames go through mdvt_mask_model_input (Pillow's Lanczos resize to the model's square and rembg's
normalize) to the planar float32 tensor the network takes, the generator is called, its prediction goes through
mdvt_mask_from_prediction (min-max stretch, bytes, Pillow's Lanczos resize to the frame's size, three equal bytes per pixel:
save_grayscale_video's frame, dfh:221-230) to the writer or the device FFV1 encoder.  Nothing is read back but the coded packets or,
with the host encoder, the finished mask frames.

The three entry points of include/mdvt_video_mask.h are bound in _lib.py and have no wrapper in the package yet (their tensor contract
records are the follow-up), so this tool hands the tensors over itself, as tools/depth_engine_video.py does."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _size(size, what):
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise ValueError(f"{what} must be (width, height) with both at least 1, got {size!r}")
    return w, h


def lanczos_resize(ctx, images, out_size, *, form=0, stream=None):
    """mdvt_lanczos_resize_u8 on uint8 CUDA images [N, H, W] (mode L) or [N, H, W, 3] (rows and frames may be strided) -> (the images
    at out_size = (w, h): Image.resize(out_size, LANCZOS) byte for byte, the form the call took: _lib.LANCZOS_FUSED,
    _lib.LANCZOS_TWO_LAUNCH or 0 for a copy).  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    _lib.check_tensor("images", images, torch.uint8, ndim=(3, 4))
    ch = 1 if images.dim() == 3 else 3
    _lib.check_tensor("images", images, torch.uint8, (None, None, None) + ((3,) if ch == 3 else ()), packed=2 if ch == 3 else 1, disjoint=True)
    N, H, W = (int(v) for v in images.shape[:3])
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f"images holds no pixel: shape {tuple(images.shape)}")
    w, h = _size(out_size, "out_size")
    dev = images.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        out = torch.empty((N, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device=dev)
    took = C.c_int(-1)
    ctx.call("mdvt_lanczos_resize_u8", W, H, ch, N, images.data_ptr(), images.stride(1), images.stride(0), w, h,
             out.data_ptr(), ch * w, ch * w * h, int(form), C.cast(C.byref(took), C.c_void_p), _lib.stream_arg(dev, s))
    return out, int(took.value)


def mask_model_input(ctx, frames, model_size, mean, std, *, bgr=False, stream=None):
    """mdvt_mask_model_input on uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided; B, G, R with bgr) -> float32
    [N, 3, h, w] at model_size = (w, h), planes R, G, B: rembg's normalize.  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    _lib.check_tensor("frames", frames, torch.uint8, (None, None, None, 3), packed=2, disjoint=True)
    N, H, W = (int(v) for v in frames.shape[:3])
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f"frames holds no pixel: shape {tuple(frames.shape)}")
    w, h = _size(model_size, "model_size")
    d3 = C.c_double * 3
    h_mean, h_std = d3(*(float(v) for v in mean)), d3(*(float(v) for v in std))
    dev = frames.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        out = torch.empty((N, 3, h, w), dtype=torch.float32, device=dev)
    ctx.call("mdvt_mask_model_input", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w, h,
             C.cast(h_mean, C.c_void_p), C.cast(h_std, C.c_void_p), out.data_ptr(), 4 * w, 4 * w * h, 12 * w * h, _lib.stream_arg(dev, s))
    return out


def mask_from_prediction(ctx, pred, out_size, *, channels=3, stream=None):
    """mdvt_mask_from_prediction on float32 CUDA planes [N, h, w] (rows and frames may be strided) -> uint8 [N, H, W, 3] (three equal
    bytes: the mask video's frame) or, with channels=1, [N, H, W] at out_size = (W, H).  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels!r}")
    _lib.check_tensor("pred", pred, torch.float32, (None, None, None), packed=1, disjoint=True)
    N, ph, pw = (int(v) for v in pred.shape)
    if N < 1 or ph < 1 or pw < 1:
        raise ValueError(f"pred holds no value: shape {tuple(pred.shape)}")
    W, H = _size(out_size, "out_size")
    dev = pred.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        out = torch.empty((N, H, W) + ((3,) if channels == 3 else ()), dtype=torch.uint8, device=dev)
    ctx.call("mdvt_mask_from_prediction", pw, ph, N, pred.data_ptr(), 4 * pred.stride(1), 4 * pred.stride(0), W, H, int(channels),
             out.data_ptr(), channels * W, channels * W * H, _lib.stream_arg(dev, s))
    return out


def checked_prediction(got, n, device):
    """What a generator returned -> float32 CUDA [n, h, w], or the TypeError / ValueError of the contract, before anything is launched on it."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    _lib.check_tensor("the generator's prediction", got, torch.float32, ndim=(3, 4), device=device)
    if got.dim() == 4:
        if got.shape[1] != 1:
            raise ValueError(f"the generator's prediction must be [n, h, w] or [n, 1, h, w], got shape {tuple(got.shape)}")
        got = got[:, 0]
    _lib.check_tensor("the generator's prediction", got, torch.float32, (n, None, None), packed=1, disjoint=True)
    if got.shape[1] < 1 or got.shape[2] < 1:
        raise ValueError(f"the generator's prediction holds no value: shape {tuple(got.shape)}")
    return got


def run_clip(args, color_video, infer):
    """gvm:65-131 for one clip -> the mask video's path."""
    import torch
    from metric_depth_video_toolbox_amd import _lib, video_mask as host
    from metric_depth_video_toolbox_amd.clip_io import ClipInputs, ClipOutput, check_video_decoder, check_video_encoder, video_parts
    with ClipInputs() as inp:
        color = inp.open(color_video, "color_video", Exception(f"input color_video does not exist: {color_video}"))     # gvm:69-70
        video = bool(video_parts(color))
        check_video_decoder(args.video_decoder, video)
        check_video_encoder(args.video_encoder, video)
        if color.ndim != 4 or color.shape[-1] != 3 or color.dtype != np.uint8:
            raise ValueError(f"{color_video}: uint8 [N, H, W, 3] expected")
        H, W = int(color.shape[1]), int(color.shape[2])
        n = host.frames_to_write(int(color.shape[0]), args.max_frames)
        if n < 1:
            raise ValueError("No frames read")
        fps = (video_parts(color)[0][0].fps or host.DEFAULT_FPS) if video else None
        tmp, final = host.output_paths(color_video, video)
        S = int(args.model_size)
        inp.on_device(torch.device("cuda", torch.cuda.current_device()), args.video_decoder, args.video_encoder)
        dev = inp.dev
        ctx = inp.ctx if inp.ctx is not None else _lib.Context(dev.index, 16, 16)
        try:
            with torch.cuda.device(dev), ClipOutput(tmp, final, n, (H, W, 3), fps, args.video_encoder, ctx) as out:
                for a in range(0, n, int(args.batch_size)):
                    b = min(n, a + int(args.batch_size))
                    x = mask_model_input(ctx, inp.fetch(color, a, b), (S, S), host.U2NET_MEAN, host.U2NET_STD)
                    pred = checked_prediction(infer(x), b - a, dev)
                    out.store(mask_from_prediction(ctx, pred, (W, H), channels=3), a)
        finally:
            if ctx is not inp.ctx:
                ctx.close()
    return final


def run(args, infer=None):
    """The step for --color_video, or for each entry of a .txt list.  infer: the generator (default: the one --generator names, loaded
    once).  -> the mask videos' paths."""
    from metric_depth_video_toolbox_amd import video_mask as host
    from metric_depth_video_toolbox_amd.infill_clip import is_txt
    host.check_flags(args)                                          # before any file is opened
    clips = host.clips_from_argument(args.color_video)
    if infer is None:
        infer = host.load_generator(args.generator)
    written = []
    for k, path in enumerate(clips, start=1):
        if len(clips) > 1 or is_txt(args.color_video):
            print(f"\n##### [{k}/{len(clips)}] {path} #####")
        written.append(run_clip(args, path, infer))
    return written


def main(argv=None):
    from metric_depth_video_toolbox_amd import video_mask as host
    for path in run(host.build_parser().parse_args(argv)):
        print(f"Done. Wrote: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
