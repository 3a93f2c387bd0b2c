#!/usr/bin/env python3
"""The reference's upscale_depth_promptda.py (pda:) around its model, on the device: a coded depth video refined against its colour
video by PromptDA.

    python tools/upscale_depth_promptda.py --color_video x.mkv --depth_video d.mkv [--max_frames N --max_depth 100 --batch 4
           --video_decoder host|device|device_all --video_encoder host|device] --generator pkg.module:callable

writes d.mkv_upscaled.mkv (tmp d.mkv_tmp_upscaled.mkv, renamed when its frame count is right; pda:84 writes the final name at
once).  .npy frame dumps give a .npy dump.  INTEGRATION.md states the generator's contract.

Per batch: the colour frames go to (ceil(W / 14) * 14, ceil(H / 14) * 14) float32 planes by mdvt_model_frames (pda:64-69: the u8 resize,
then / 255), the 256 x 192 prompt comes from mdvt_depth_prompt (pda:59-62, the decode fused into the resize's gathers), the model is
called, and mdvt_depth_video_codes resizes its output to (W, H) and codes it (pda:77-84: the script's own resize and
save_depth_video's, which then has nothing left to do, are that one resize).  The model's size is less than 14 pixels above the frame's, so from
14 x 14 frames on the sink meets no exact-2x case; a depth video of exactly 512 x 384 would be one for the prompt and is refused by mdvt_depth_prompt.

The loop ends with the shorter of the two videos (pda:51-58): step_clip.py's clip session opens both, holds them to one kind and
counts the shorter one; the three device wrappers are metric_depth_video_toolbox_amd/step_device.py's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def checked_upscale(got, n, h14, w14):
    """What a generator returned -> depth float32 CUDA [n, h14, w14], or the TypeError / ValueError of the contract."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    return _lib.check_tensor("the generator's depth", got, torch.float32, (n, h14, w14), packed=1, disjoint=True)


def run(args, upscale=None):
    """pda:30-84 for one pair of clips -> the upscaled depth video's path."""
    from metric_depth_video_toolbox_amd import depth_engines as host, step_clip
    from metric_depth_video_toolbox_amd.step_device import depth_prompt, depth_video_codes, model_frames
    if int(args.batch) < 1:
        raise ValueError(f"--batch must be at least 1, got {args.batch}")
    if upscale is None:
        upscale = host.load_generator(args.generator, "promptda")
    with step_clip.StepClip() as clip:
        # the session's checks for two inputs: both .mkv or both .npy; the shorter of the two counts (pda:51-58); the colour video's rate (pda:33)
        color, depth = clip.open_checked([(args.color_video, "color_video", Exception("input color_video does not exist")),
                                          (args.depth_video, "depth_video", Exception("input depth_video does not exist"))],
                                         args.video_decoder, args.video_encoder, lambda n: host.frames_to_write(n, args.max_frames),
                                         label="--{name}")
        n, H, W = clip.n, clip.H, clip.W
        h14, w14 = host.closest_higher_multiple(H), host.closest_higher_multiple(W)          # pda:38
        tmp, final = host.promptda_output_paths(args.depth_video, clip.video)
        with clip.device(tmp, final) as (ctx, fetch, store):
            for a in range(0, n, int(args.batch)):
                b = min(n, a + int(args.batch))
                rgb = model_frames(ctx, fetch(color, a, b), (w14, h14), as_float=True)
                prompt = depth_prompt(ctx, fetch(depth, a, b), args.max_depth, (host.PROMPT_W, host.PROMPT_H))
                up = checked_upscale(upscale(rgb, prompt.unsqueeze(1)), b - a, h14, w14)
                store(depth_video_codes(ctx, up, args.max_depth, (W, H)), a)
    return final


def main(argv=None):
    from metric_depth_video_toolbox_amd import depth_engines as host
    print(f"saved: {run(host.build_promptda_parser().parse_args(argv))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
