#!/usr/bin/env python3
"""Step 0 of the reference's movie_2_3D.py (m23d:209-222 runs `scenedetect -i movie list-scenes`), on the device: the scene list of a
video as PySceneDetect's `<video stem>-Scenes.csv`.

    python tools/scene_detect.py --color_video x.mkv|x.npy [--detector adaptive|content --threshold 27 --adaptive_threshold 3
           --min_content_val 15 --min_scene_len 15 --downscale auto|N --fps F --batch 64
           --video_decoder host|device|device_all --output x-Scenes.csv]

The detectors, the CSV and the parser are host logic in metric_depth_video_toolbox_amd/scene_detect.py (restated PySceneDetect
0.6.x defaults: a decree, README); the opening of the clip with its checks and the context are step_clip.py's.  Here is what
touches the device: per batch the decoded frames go through mdvt_scene_frame_sums (include/mdvt_scene.h) together with the last
frame of the batch before, and 24 bytes per frame pair are read back.  frame_sums, the wrapper of that entry point, is
metric_depth_video_toolbox_amd/step_device.py's; it stays reachable under this module's name.  The file is written under a temporary
name and renamed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metric_depth_video_toolbox_amd.step_device import frame_sums      # noqa: E402


def run_clip(args):
    """The scene list of one clip -> (the CSV's path, [(first frame, frame behind the last)])."""
    from metric_depth_video_toolbox_amd import scene_detect as host, step_clip
    host.check_flags(args)
    with step_clip.StepClip() as clip:
        color, = clip.open_checked([(args.color_video, "color_video", FileNotFoundError(f"input color_video does not exist: {args.color_video}"))],
                                   args.video_decoder, "host", lambda n: n, default_fps=30.0)
        fps = float(args.fps) if args.fps is not None and (not clip.video or not step_clip.video_parts(color)[0][0].fps) else clip.fps
        if fps is None:
            raise ValueError("--fps is needed with a .npy frame dump, which states no frame rate")
        factor = host.downscale_factor(args.downscale, clip.W, clip.H)
        pixels = host.analysed_pixels(clip.W, clip.H, factor)
        out = args.output or host.scene_file_path(args.color_video, os.path.dirname(args.color_video))
        import torch
        clip.on_device(torch.device("cuda", torch.cuda.current_device()), args.video_decoder, "host", own_context=True)
        sums, prev = [], None
        with torch.cuda.device(clip.dev):
            for a in range(0, clip.n, int(args.batch)):
                b = min(clip.n, a + int(args.batch))
                frames = clip.fetch(color, a, b)
                if prev is not None or b - a > 1:
                    sums.extend(frame_sums(clip.ctx, frames, prev, factor).cpu().tolist())        # 24 bytes per pair
                prev = frames[-1]
    scores = host.scores_from_sums(sums, pixels)
    cuts = host.detect_cuts(scores, args.detector, args.threshold, args.adaptive_threshold, args.min_content_val, args.min_scene_len)
    scenes = host.scenes_from_cuts(cuts, clip.n)
    host.write_scene_csv(out, scenes, fps)
    return out, scenes


def main(argv=None):
    from metric_depth_video_toolbox_amd import scene_detect as host
    out, scenes = run_clip(host.build_parser().parse_args(argv))
    print(f"Done. Wrote: {out}  ({len(scenes)} scenes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
