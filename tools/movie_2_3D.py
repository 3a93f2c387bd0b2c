#!/usr/bin/env python3
"""The reference's movie_2_3D.py (m23d:785-830) on the device: a movie to an infilled side-by-side movie, scene by scene.

    python tools/movie_2_3D.py --color_video movie.mkv [--scene_file movie-Scenes.csv --csv_delimiter , --output_dir output
           --end_scene N --no_render --max_scene_frames 1500 --infill_engine none|normals|stereocrafter|m2svid|stereo_dissoclusion_net
           --video_decoder host|device|device_all --video_encoder host|device
           --depth_generator pkg.module:callable --mask_generator pkg.module:callable --infill_generator pkg.module:callable]

Step 0 lists the scenes (tools/scene_detect.py) where no --scene_file is given; step 1 cuts the movie into scene_N.mkv; steps 2-6
call each step's own main(argv) in this process, one after another, skipping what the reference's file-existence rules skip, so a
rerun resumes; step 7 joins the per-scene results into <output_dir>/<movie name>_SBS.mkv (FFV1; tmp, then rename, the frame count
verified against the scene list) and prints the ffmpeg line that would mux the movie's audio onto it.  The plan -- scene chunks,
file names, every step's argv -- is host logic in metric_depth_video_toolbox_amd/movie_2_3D.py."""
import importlib
import importlib.util
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

TOOL_FILES = ("scene_detect", "video_da3", "depth_engine_video", "generate_video_mask")      # tools/ scripts; the others are package modules
_mains = {}


def tool_main(name):
    """main(argv) of a step: a script of tools/ or a module of the package."""
    if name not in _mains:
        if name in TOOL_FILES:
            spec = importlib.util.spec_from_file_location("mdvt_tool_" + name, os.path.join(HERE, name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        else:
            mod = importlib.import_module("metric_depth_video_toolbox_amd." + name)
        _mains[name] = mod.main
    return _mains[name]


def write_clip(inp, parts, tmp, final, frame_shape, fps, codecs, batch=32):
    """Frames [a, b) of every (frames, a, b) of parts, in order, into one video: tmp, then renamed when its frame count is right."""
    import numpy as np
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    n = sum(b - a for _, a, b in parts)
    on_host = codecs == ("host", "host")
    with ClipOutput(tmp, final, n, frame_shape, fps, codecs[1], inp.ctx) as out:
        at = 0
        for frames, a, b in parts:
            for lo in range(a, b, batch):
                hi = min(b, lo + batch)
                if on_host:
                    out.sink.write_from(np.ascontiguousarray(frames[lo:hi]), at, hi - lo)
                else:
                    out.store(inp.fetch(frames, lo, hi), at)
                at += hi - lo
    return n


def _on_device(inp, codecs):
    if codecs != ("host", "host"):
        import torch
        inp.on_device(torch.device("cuda", torch.cuda.current_device()), *codecs)


def step1_scene_clips(args, scenes, log):
    """m23d:283-301: scene_N.mkv for every scene that is not finished and has none; the frames are the scene list's own ranges."""
    from metric_depth_video_toolbox_amd.clip_io import ClipInputs, check_video_decoder, check_video_encoder, video_parts
    todo = [s for s in scenes if not s["finished"] and not os.path.exists(s["scene_video_file"])]
    if not todo:
        return
    codecs = (args.video_decoder, args.video_encoder)
    with ClipInputs() as inp:
        movie = inp.open(args.color_video, "color_video", FileNotFoundError(f"input color_video does not exist: {args.color_video}"))
        if not video_parts(movie):
            raise ValueError(f"{args.color_video}: --color_video must be an .mkv file")
        check_video_decoder(codecs[0], True)
        check_video_encoder(codecs[1], True)
        n, H, W = (int(v) for v in movie.shape[:3])
        fps = video_parts(movie)[0][0].fps or 30.0
        for s in todo:
            a, b = int(s["Start Frame"]) - 1, int(s["End Frame"])
            if not (0 <= a < b <= n) or b - a != int(s["Length (frames)"]):
                raise ValueError(f"scene {s['Scene Number']}: frames {a + 1}..{b} ({s['Length (frames)']} long) do not lie in a movie of {n} frames")
        _on_device(inp, codecs)
        for s in todo:
            print("create:", s["scene_video_file"])
            write_clip(inp, [(movie, int(s["Start Frame"]) - 1, int(s["End Frame"]))], s["scene_video_file"] + "_tmp.mkv", s["scene_video_file"],
                       (H, W, 3), fps, codecs)
            log.append((1, s["Scene Number"], "scene_clip"))


def run_commands(args, scenes, log):
    """Steps 2-6, step by step over the scenes as the reference goes (m23d:806-821)."""
    from metric_depth_video_toolbox_amd import movie_2_3D as host
    plans = [(s, host.plan_commands(s, args)) for s in scenes]
    for step in (2, 3, 4, 5, 6):
        for s, cmds in plans:
            for c in cmds:
                if c.step != step or os.path.exists(c.skip_if_exists):
                    continue
                argv = list(c.argv)
                if c.xfov_from is not None:
                    with open(c.xfov_from) as fh:
                        xfovs = json.load(fh)
                    xfov = float(sum(float(v) for v in xfovs) / len(xfovs))
                    argv = [str(xfov) if a == host.XFOV_TOKEN else a for a in argv]
                print(f"step {step}, scene {s['Scene Number']}: {c.tool} {' '.join(argv)}")
                tool_main(c.tool)(argv)
                if c.move is not None:
                    shutil.move(*c.move)
                if not os.path.exists(c.skip_if_exists):
                    raise RuntimeError(f"step {step}, scene {s['Scene Number']}: {c.tool} did not write {c.skip_if_exists}")
                log.append((step, s["Scene Number"], c.tool))


def step7_join(args, scenes, log, force):
    """The per-scene results joined into <output_dir>/<movie name>_SBS.mkv; every file's frame count is the scene list's."""
    from metric_depth_video_toolbox_amd import movie_2_3D as host
    from metric_depth_video_toolbox_amd.clip_io import ClipInputs, frames_in, video_parts
    result = host.result_path(args)
    if os.path.exists(result) and not force:
        return result
    files = [host.file_to_concat(s, args) for s in scenes]
    for s, f in zip(scenes, files):                                                           # m23d:70-100
        if not os.path.isfile(f):
            raise FileNotFoundError(f"scene file is missing: {f}")
        if frames_in(f) != int(s["Length (frames)"]):
            raise RuntimeError(f"{f}: {frames_in(f)} frames, the scene list says {s['Length (frames)']}; delete it and run again")
    codecs = (args.video_decoder, args.video_encoder)
    with ClipInputs() as inp:
        parts = [inp.open(f, "scene", FileNotFoundError(f)) for f in files]
        shape = tuple(int(v) for v in parts[0].shape[1:])
        if any(tuple(int(v) for v in p.shape[1:]) != shape for p in parts):
            raise ValueError("the scenes' side-by-side videos differ in size")
        fps = video_parts(parts[0])[0][0].fps or 30.0
        _on_device(inp, codecs)
        write_clip(inp, [(p, 0, int(p.shape[0])) for p in parts], result[:-4] + "_tmp.mkv", result, shape, fps, codecs)
    log.append((7, "all", "join"))
    print("To mux the movie's audio onto it:\n  " + host.mux_line(args))
    return result


def run(args):
    """The whole pipeline -> (the joined file's path or None with --no_render, the log [(step, scene, tool)] of what ran)."""
    from metric_depth_video_toolbox_amd import movie_2_3D as host
    host.check_args(args)
    if not os.path.isfile(args.color_video):
        raise FileNotFoundError(f"input color_video does not exist: {args.color_video}")
    if args.scene_file is not None and not os.path.isfile(args.scene_file):
        raise FileNotFoundError(f"scene file does not exist: {args.scene_file}")
    log = []
    os.makedirs(args.output_dir, exist_ok=True)                                               # m23d:204-206
    if args.scene_file is None:                                                               # m23d:209-222
        args.scene_file = host.scene_file_path(args.color_video, args.output_dir)
        if not os.path.exists(args.scene_file):
            tool_main("scene_detect")(["--color_video", args.color_video, "--output", args.scene_file, "--video_decoder", args.video_decoder])
            log.append((0, "all", "scene_detect"))
    scenes = host.plan_scene_files(host.load_and_split_scenes(args.scene_file, args.csv_delimiter, args.max_scene_frames),
                                   args.output_dir, args.end_scene)
    for s in scenes:
        host.plan_commands(s, args)                      # an unknown Engine is refused before a scene clip is written
    step1_scene_clips(args, scenes, log)
    run_commands(args, scenes, log)
    if args.no_render:
        return None, log
    return step7_join(args, scenes, log, force=any(step >= 5 for step, _, _ in log)), log


def main(argv=None):
    from metric_depth_video_toolbox_amd import movie_2_3D as host
    result, _ = run(host.build_parser().parse_args(argv))
    if result is not None:
        print(f"Done. Wrote: {result}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
