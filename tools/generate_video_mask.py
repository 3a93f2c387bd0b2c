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

lanczos_resize, mask_model_input and mask_from_prediction, the wrappers of include/mdvt_video_mask.h's three entry points, are
metric_depth_video_toolbox_amd/step_device.py's; they stay reachable under this module's name."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metric_depth_video_toolbox_amd.step_device import lanczos_resize, mask_from_prediction, mask_model_input      # noqa: E402, F401


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
