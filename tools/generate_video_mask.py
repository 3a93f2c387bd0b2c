#!/usr/bin/env python3
"""The reference's generate_video_mask.py (gvm:) around its model, on the device: step 3 of movie_2_3D.py, which writes the black and
white video of the main subject that find_convergence_depth --mask_video and stereo_rerender --convergence_mask_video read.

    python tools/generate_video_mask.py --color_video x.mkv|list.txt [--max_frames N --batch_size 8 --model_size 320
           --video_decoder host|device|device_all --video_encoder host|device] [--generator pkg.module:callable]

writes x.mkv_mask.mkv (tmp x.mkv_tmp_mask.mkv, renamed when its frame count is right).  A .txt list runs each entry; a .npy frame dump
gives a .npy mask.  INTEGRATION.md states the generator's contract.

The parser, the file names and U2-Net's constants are host logic in metric_depth_video_toolbox_amd/video_mask.py; the opening of the
clip with its checks, the context, the output file and the list loop are step_clip.py's.  Here is what touches the device, per
batch: the decoded frames go through mdvt_mask_model_input (Pillow's Lanczos resize to the model's square and rembg's normalize)
to the planar float32 tensor the network takes, the generator is called, its prediction goes through mdvt_mask_from_prediction (min-max stretch, bytes, Pillow's Lanczos resize to the frame's size, three equal bytes per pixel:
save_grayscale_video's frame, dfh:221-230) to the writer or the device FFV1 encoder.  Nothing is read back but the coded packets or,
with the host encoder, the finished mask frames.

The three entry points of include/mdvt_video_mask.h are bound in _lib.py and have no wrapper in the package yet (their tensor contract
records are the follow-up), so this tool hands the tensors over itself, as tools/depth_engine_video.py does."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def lanczos_resize(ctx, images, out_size, *, form=0, stream=None):
    """mdvt_lanczos_resize_u8 on uint8 CUDA images [N, H, W] (mode L) or [N, H, W, 3] (rows and frames may be strided) -> (the images
    at out_size = (w, h): Image.resize(out_size, LANCZOS) byte for byte, the form the call took: _lib.LANCZOS_FUSED,
    _lib.LANCZOS_TWO_LAUNCH or 0 for a copy).  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib, step_clip
    _lib.check_tensor("images", images, torch.uint8, ndim=(3, 4))
    ch = 1 if images.dim() == 3 else 3
    _lib.check_tensor("images", images, torch.uint8, (None, None, None) + ((3,) if ch == 3 else ()), packed=2 if ch == 3 else 1, disjoint=True)
    N, H, W = step_clip.non_empty("images", images, "pixel")
    w, h = step_clip.size_arg(out_size, "out_size")
    dev = images.device
    s = step_clip.stream_or_current(dev, stream)
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
    from metric_depth_video_toolbox_amd import _lib, step_clip
    _lib.check_tensor("frames", frames, torch.uint8, (None, None, None, 3), packed=2, disjoint=True)
    N, H, W = step_clip.non_empty("frames", frames, "pixel")
    w, h = step_clip.size_arg(model_size, "model_size")
    d3 = C.c_double * 3
    h_mean, h_std = d3(*(float(v) for v in mean)), d3(*(float(v) for v in std))
    dev = frames.device
    s = step_clip.stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, 3, h, w), dtype=torch.float32, device=dev)
    ctx.call("mdvt_mask_model_input", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w, h,
             C.cast(h_mean, C.c_void_p), C.cast(h_std, C.c_void_p), out.data_ptr(), 4 * w, 4 * w * h, 12 * w * h, _lib.stream_arg(dev, s))
    return out


def mask_from_prediction(ctx, pred, out_size, *, channels=3, stream=None):
    """mdvt_mask_from_prediction on float32 CUDA planes [N, h, w] (rows and frames may be strided) -> uint8 [N, H, W, 3] (three equal
    bytes: the mask video's frame) or, with channels=1, [N, H, W] at out_size = (W, H).  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib, step_clip
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, got {channels!r}")
    _lib.check_tensor("pred", pred, torch.float32, (None, None, None), packed=1, disjoint=True)
    N, ph, pw = step_clip.non_empty("pred", pred, "value")
    W, H = step_clip.size_arg(out_size, "out_size")
    dev = pred.device
    s = step_clip.stream_or_current(dev, stream)
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
    from metric_depth_video_toolbox_amd import step_clip, video_mask as host
    with step_clip.StepClip() as clip:
        color, = clip.open_checked([(color_video, "color_video", Exception(f"input color_video does not exist: {color_video}"))],   # gvm:69-70
                                   args.video_decoder, args.video_encoder, lambda n: host.frames_to_write(n, args.max_frames),
                                   default_fps=host.DEFAULT_FPS)
        tmp, final = host.output_paths(color_video, clip.video)
        S = int(args.model_size)
        with clip.device(tmp, final) as (ctx, fetch, store):
            for a in range(0, clip.n, int(args.batch_size)):
                b = min(clip.n, a + int(args.batch_size))
                x = mask_model_input(ctx, fetch(color, a, b), (S, S), host.U2NET_MEAN, host.U2NET_STD)
                pred = checked_prediction(infer(x), b - a, clip.dev)
                store(mask_from_prediction(ctx, pred, (clip.W, clip.H), channels=3), a)
    return final


def run(args, infer=None):
    """The step for --color_video, or for each entry of a .txt list.  infer: the generator (default: the one --generator names, loaded
    once).  -> the mask videos' paths."""
    from metric_depth_video_toolbox_amd import step_clip, video_mask as host
    return step_clip.run_list(args, infer, host.check_flags, lambda: host.load_generator(args.generator), run_clip,
                              banner="\n##### [{k}/{n}] {path} #####")


def main(argv=None):
    from metric_depth_video_toolbox_amd import video_mask as host
    for path in run(host.build_parser().parse_args(argv)):
        print(f"Done. Wrote: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
