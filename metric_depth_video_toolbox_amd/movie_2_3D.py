"""Host side of the reference's movie_2_3D.py (m23d:): the scene list split into chunks, the per-scene file names, and the argv of
every step of a scene.  Importable without torch; nothing here touches a GPU or runs a step (tools/movie_2_3D.py does).

    split_scenes(scenes, max_scene_frames)        m23d:111-173
    plan_scene_files(scenes, output_dir, end)     m23d:244-280
    plan_commands(scene, args)                    the argv list of steps 2-6 for one scene, as m23d:304-700 composes them

What differs from the reference, by decree (README, DESIGN.md "movie_2_3D"):
  - the steps run in this process one after another (the GPU is the worker); --parallel is parsed and unused;
  - the models stand behind --depth_generator / --mask_generator / --infill_generator (each tool's --generator);
  - vda, depthcrafter and geometrycrafter go through video_metric_convert, which takes the model's relative depth as a dump
    `<scene>_relative_depth.npy` (and, for vda, the metric reference `<scene>_metric_depth.npy`): the models themselves are not
    this project's; geometrycrafter takes depthcrafter's clean-up rule;
  - an Engine of unik3d, moge or depthpro writes the scene's depth video itself, as the single-frame reference does;
  - stereo_dissoclusion_net reads `<sbs>_depth.mkv`, which the render writes for it (--create_sbs_depth_video): the reference
    names a key it never sets (m23d:689);
  - step 7 joins the per-scene files into `<output_dir>/<movie name>_SBS.mkv` (FFV1); the libx264 / audio mux needs FFmpeg.
"""
from __future__ import annotations

import argparse
import os
from collections import namedtuple

from .scene_detect import load_scene_csv, scene_file_path, timecode

INFILL_ENGINES = ("none", "normals", "stereo_dissoclusion_net", "stereocrafter", "m2svid")
INSPATIO_REASON = ("--infill_engine inspatio_world is left out: its alignment is scikit-image's masked phase correlation, which "
                   "cannot be pinned here")
METRIC_CONVERT_ENGINES = ("vda", "depthcrafter", "geometrycrafter")
SINGLE_FRAME_ENGINES = ("unik3d", "moge", "depthpro")
DEPTH_ENGINES = ("da3",) + METRIC_CONVERT_ENGINES + SINGLE_FRAME_ENGINES
XFOV_TOKEN = "{xfov}"                                    # stands in an argv for the mean of the x-fovs file the command names

# step: 2 .. 6; tool: the module whose main(argv) runs; skip_if_exists: the file whose existence skips the command;
# move: (src, dst) renamed after the command; xfov_from: the x-fovs JSON whose mean replaces XFOV_TOKEN in argv
Command = namedtuple("Command", "step tool argv skip_if_exists move xfov_from", defaults=(None, None))


def split_scenes(scenes, max_scene_frames: int = 1500):
    """m23d:111-173: scenes longer than max_scene_frames in chunks, every other key kept, 'Scene Number' renumbered from 1."""
    out = []
    for scene in scenes:
        sf, ef = int(scene["Start Frame"]), int(scene["End Frame"])
        ss, es = float(scene["Start Time (seconds)"]), float(scene["End Time (seconds)"])
        spf = (es - ss) / (ef - sf) if ef != sf else 0.0

        def chunk(a, b, scene=scene, sf=sf, ss=ss, spf=spf):
            t0, t1 = ss + (a - sf) * spf, ss + (b - sf) * spf
            d = dict(scene)
            d.update({"Scene Number": None, "Start Frame": str(a), "Start Time (seconds)": f"{t0:.3f}", "Start Timecode": timecode(t0),
                      "End Frame": str(b), "End Time (seconds)": f"{t1:.3f}", "End Timecode": timecode(t1),
                      "Length (frames)": str(b - a + 1), "Length (seconds)": f"{max(0.0, t1 - t0):.3f}",
                      "Length (timecode)": timecode(max(0.0, t1 - t0))})
            return d
        length = ef - sf + 1
        if length <= max_scene_frames:                   # (a scene of no or negative length is kept as it is, m23d:150-153)
            out.append(chunk(sf, ef))
            continue
        a = sf
        while a <= ef:
            b = min(ef, a + max_scene_frames - 1)
            out.append(chunk(a, b))
            a = b + 1
    for k, d in enumerate(out, start=1):
        d["Scene Number"] = str(k)
    return out


def load_and_split_scenes(scene_csv_path: str, csv_delimiter: str, max_scene_frames: int):
    """m23d:233-241."""
    return split_scenes(load_scene_csv(scene_csv_path, csv_delimiter), max_scene_frames=max_scene_frames)


def plan_scene_files(scenes, output_dir: str, end_scene: int, exists=os.path.exists):
    """m23d:244-280: the per-scene file names and flags, into the scene dicts; the list ends behind scene `end_scene`."""
    out = []
    for scene in scenes:
        base = os.path.join(output_dir, f"scene_{scene['Scene Number']}.mkv")
        scene["scene_video_file"] = base
        scene["depth_video_file"] = base + "_depth.mkv"
        scene["mask_video_file"] = base + "_mask.mkv"
        scene["xfovs_file"] = scene["depth_video_file"] + "_xfovs.json"
        scene["sbs"] = scene["depth_video_file"] + "_stereo.mkv"
        scene["sbs_infill"] = scene["sbs"] + "_infillmask.mkv"
        scene["infilled"] = scene["sbs"] + "_infilled.mkv"
        scene["infill"] = not ("Infill" in scene and scene["Infill"] == "No")
        scene["convergence"] = not ("Convergence" in scene and scene["Convergence"] == "No")
        scene["finished"] = exists(scene["sbs"]) or exists(scene["infilled"])
        out.append(scene)
        if end_scene == int(scene["Scene Number"]):
            break
    return out


def depth_engine_of(scene) -> str:
    """m23d:326-328: the 'Engine' column, da3 where there is none."""
    engine = scene.get("Engine") or "da3"
    if engine not in DEPTH_ENGINES:
        raise ValueError(f"scene {scene.get('Scene Number')}: Engine must be one of {DEPTH_ENGINES}, got {engine!r}")
    return engine


def do_infill(scene, args) -> bool:
    return args.infill_engine != "none" and bool(scene.get("infill", True))


def file_to_concat(scene, args) -> str:
    """The scene's file that step 7 joins (m23d:486-495)."""
    return scene["infilled"] if do_infill(scene, args) else scene["sbs"]


def check_args(args):
    """What is refused before anything is written."""
    if getattr(args, "gui", False):
        raise NotImplementedError("--gui is refused: the PySide6 front end is outside this project (SURVEY: out of scope)")
    if args.color_video is None:
        raise ValueError("need --color_video")               # m23d:198-199
    if args.infill_engine == "inspatio_world":
        raise NotImplementedError(INSPATIO_REASON)
    if args.infill_engine not in INFILL_ENGINES:
        raise ValueError(f"unknown infill engine: {args.infill_engine}")      # m23d:467
    if int(args.max_scene_frames) < 1:
        raise ValueError("--max_scene_frames must be >= 1")


def _codec(args, decoder=True, encoder=True):
    out = []
    if decoder and getattr(args, "video_decoder", "host") != "host":
        out += ["--video_decoder", args.video_decoder]
    if encoder and getattr(args, "video_encoder", "host") != "host":
        out += ["--video_encoder", args.video_encoder]
    return out


def _gen(args, which):
    spec = getattr(args, which + "_generator", None)
    return ["--generator", spec] if spec else []


def plan_commands(scene, args):
    """The commands of steps 2-6 for one planned scene, in order, as m23d:304-700 composes them; a pure function of its arguments.
    A finished scene (m23d:270) takes none of steps 2-5.  The runner skips a command whose skip_if_exists file exists."""
    if args.infill_engine == "inspatio_world":
        raise NotImplementedError(INSPATIO_REASON)
    if args.infill_engine not in INFILL_ENGINES:
        raise ValueError(f"unknown infill engine: {args.infill_engine}")
    engine = depth_engine_of(scene)
    video, depth, mask = scene["scene_video_file"], scene["depth_video_file"], scene["mask_video_file"]
    cmds = []
    xfov_args = ["--xfov_file", scene["xfovs_file"]]
    xfov_from = None
    if not scene["finished"]:
        dgen, codec = _gen(args, "depth"), _codec(args)
        if engine == "da3":                                                                   # m23d:354-358, 382-383
            cmds.append(Command(2, "video_da3", ["--color_video", video] + dgen + codec, depth))
        elif engine in SINGLE_FRAME_ENGINES:
            cmds.append(Command(2, "depth_engine_video", ["--engine", engine, "--color_video", video] + dgen + codec, depth))
        else:
            rel = video + "_relative_depth.npy"
            if engine == "vda":                                                               # m23d:350-351, 359-363, 378-379
                xfov_args = ["--xfov", "42.0"]
                ref = ["--metric_depth", video + "_metric_depth.npy"]
            else:                                                                             # m23d:333-347, 366-373
                org, single = depth + "_org_xfovs.json", video + "_single_frame_depth.mkv"
                cmds.append(Command(2, "depth_engine_video", ["--engine", "unik3d", "--color_video", video] + dgen + codec,
                                    org, (scene["xfovs_file"], org)))
                cmds.append(Command(2, "depth_engine_video", ["--engine", "unik3d", "--xfov", XFOV_TOKEN, "--color_video", video] + dgen + codec,
                                    single, (depth, single), org))
                xfov_args, xfov_from = ["--xfov", XFOV_TOKEN], org
                ref = ["--depth_video", single]
            cmds.append(Command(2, "video_metric_convert",
                                ["--color_video", video, "--relative_depth", rel] + ref + ["--engine", "vda" if engine == "vda" else "depthcrafter"] + codec,
                                depth))
        cmds.append(Command(3, "generate_video_mask", ["--color_video", video] + _gen(args, "mask") + codec, mask))       # m23d:397-404
        conv = depth + "_convergence_depths.json"                                             # m23d:417-419
        cmds.append(Command(4, "find_convergence_depth", ["--depth_video", depth, "--mask_video", mask] + _codec(args, encoder=False), conv))
        if not getattr(args, "no_render", False):                                             # m23d:430-446
            argv = ["--color_video", video]
            if scene.get("convergence", True):
                argv += ["--convergence_file", conv]
            argv += xfov_args + ["--depth_video", depth]
            if scene.get("infill", True):
                argv += ["--infill_mask"]
            if args.infill_engine == "stereo_dissoclusion_net" and do_infill(scene, args):
                argv += ["--create_sbs_depth_video"]
            cmds.append(Command(5, "stereo_rerender", argv + codec, scene["sbs"], None, xfov_from))
    if getattr(args, "no_render", False) or not do_infill(scene, args):
        return cmds
    pair = ["--sbs_color_video", scene["sbs"], "--sbs_mask_video", scene["sbs_infill"]]
    igen, codec = _gen(args, "infill"), _codec(args)
    if args.infill_engine == "normals":                                                       # m23d:491-493
        cmds.append(Command(6, "basic_nomal_infill", pair + codec, scene["infilled"]))
    elif args.infill_engine == "stereocrafter":                                               # m23d:646-647
        cmds.append(Command(6, "stereo_crafter_infill", pair + igen + codec, scene["infilled"]))
    elif args.infill_engine == "m2svid":                                                      # m23d:545-546
        cmds.append(Command(6, "m2svid_infill", ["--color_video", video] + pair + igen + codec, scene["infilled"]))
    else:                                                                                     # m23d:693-694
        cmds.append(Command(6, "stereo_dissoclusion_net_infill", pair + ["--sbs_depth_video", scene["sbs"] + "_depth.mkv"] + igen + codec,
                            scene["infilled"]))
    return cmds


def result_path(args) -> str:
    """`<output_dir>/<movie name>_SBS.mkv` (the reference's name, m23d:720-721, with this project's container)."""
    return os.path.join(args.output_dir, os.path.basename(args.color_video) + "_SBS.mkv")


def mux_line(args) -> str:
    """The one ffmpeg line that would put the movie's audio onto the joined file (what m23d:752-762 does while it encodes)."""
    out = result_path(args)
    return (f"ffmpeg -y -i {out} -i {args.color_video} -metadata:s:v:0 stereo_mode=left_right -x264opts \"frame-packing=3\" "
            f"-map 0:v:0 -map 1:a:0 -c:a copy -shortest -c:v libx264 -crf 18 -preset veryfast -pix_fmt yuv420p {out[:-4]}.mp4")


def build_parser():
    from .clip_io import VIDEO_DECODERS, VIDEO_ENCODERS
    p = argparse.ArgumentParser(description="Takes a movie and converts it in to stereo 3D")
    p.add_argument("--color_video", type=str, default=None, help="video file to use as color input (.mkv with FFV1)")
    p.add_argument("--scene_file", type=str, default=None, help="csv from PySceneDetect describing the scenes (default: made by step 0)")
    p.add_argument("--csv_delimiter", type=str, default=",", help="Delimiter used in csv")
    p.add_argument("--output_dir", type=str, default="output", help="folder where output will be placed")
    p.add_argument("--end_scene", type=int, default=-1, help="Stop after a certain scene nr")
    p.add_argument("--no_render", action="store_true", help="Skip rendering and subseqvent steps.")
    p.add_argument("--parallel", type=int, default=1, help="parsed and unused: the steps run one after another on the GPU")
    p.add_argument("--max_scene_frames", type=int, default=1500, help="Max length of scene in nr of frames, longer scenes will be processed in chunks.")
    p.add_argument("--infill_engine", type=str, default="stereocrafter",
                   help="What infill engine to use. (none, normals, stereo_dissoclusion_net, stereocrafter, m2svid)")
    p.add_argument("--gui", action="store_true", help="refused: the GUI is outside this project")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host", help="not a reference flag: handed to every step that reads an .mkv")
    p.add_argument("--video_encoder", choices=VIDEO_ENCODERS, default="host", help="not a reference flag: handed to every step that writes an .mkv")
    for which, step in (("depth", "the depth step (2)"), ("mask", "the mask step (3)"), ("infill", "the infill step (6)")):
        p.add_argument(f"--{which}_generator", type=str, default=None, help=f"not a reference flag: the --generator of {step}")
    return p


__all__ = ["Command", "XFOV_TOKEN", "split_scenes", "load_and_split_scenes", "plan_scene_files", "plan_commands", "check_args",
           "file_to_concat", "result_path", "mux_line", "build_parser", "scene_file_path"]
