#!/usr/bin/env python3
"""The reference's per-frame depth engines around their models, on the device: unik3d_video.py (u3d:), moge_video.py (mge:) and
depthpro_video.py (dpr:), the step movie_2_3D.py:333-347 runs twice per scene in front of DepthCrafter's and GeometryCrafter's
metric conversion.

    python tools/depth_engine_video.py --engine unik3d|moge|depthpro --color_video x.mkv|list.txt [--max_frames N --max_depth 100
           --xfov F --yfov F --batch 8 --video_decoder host|device|device_all --video_encoder host|device] --generator pkg.module:callable

writes x.mkv_depth.mkv (tmp x.mkv_tmp_depth.mkv, renamed when its frame count is right) and x.mkv_depth.mkv_xfovs.json.  A .txt list
runs each entry; a .npy frame dump gives .npy depth frames.  INTEGRATION.md states the generator's contract.

The parsers, the file names and the x-fov arithmetic are host logic in metric_depth_video_toolbox_amd/depth_engines.py; the opening
of the clip with its checks, the context, the output file and the list loop are step_clip.py's.  Here is what touches the device,
per batch: the decoded frames go through mdvt_model_frames to the planar tensor the model takes (uint8 for unik3d
and depthpro, float32 / 255 for moge), the model is called, unik3d's point map goes through mdvt_focal_from_points, ONE read-back
brings the batch's focal lengths (8 bytes per frame) or intrinsics to the host for the x-fov list, and the depth goes through
mdvt_depth_video_codes (with moge's NaN rule, mge:171) to the writer or the device FFV1 encoder.

moge and depthpro write through their own save_24bit (mge:68-102, dpr:62-96), which does not clip.  It equals the sink's code for
every depth in [0, max_depth] and has no defined result outside (a float64 out of uint32's range).  DECREE: those depths take the
sink's clip, like every other depth video of this project.

model_frames, depth_prompt and focal_from_points, the wrappers of include/mdvt_depth_engines.h's three entry points, are
metric_depth_video_toolbox_amd/step_device.py's; they stay reachable under this module's name."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metric_depth_video_toolbox_amd.step_device import depth_prompt, focal_from_points, model_frames      # noqa: E402, F401


def sibling_tool(name):
    """tools/<name>.py as a module, loaded once."""
    key = "mdvt_tool_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(HERE, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[key] = mod
        spec.loader.exec_module(mod)
    return sys.modules[key]


def checked_prediction(got, engine, n, W, H):
    """What a generator returned -> (depth float32 CUDA [n, h, w], the engine's second tensor), or the TypeError / ValueError of the
    contract, before anything is launched on it."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    second = {"unik3d": "points", "moge": "intrinsics", "depthpro": "focallength_px"}[engine]
    if not isinstance(got, dict) or "depth" not in got or second not in got:
        raise TypeError(f"the {engine} generator must return a dict with 'depth' and '{second}'")
    depth = got["depth"]
    _lib.check_tensor("the generator's depth", depth, torch.float32, (n, None, None), packed=1, disjoint=True)
    if depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"the generator's depth holds no value: shape {tuple(depth.shape)}")
    extra = got[second]
    if engine == "unik3d":
        _lib.check_tensor("the generator's points", extra, torch.float32, ndim=4, device=depth.device)
        if tuple(extra.shape) not in ((n, H, W, 3), (n, 3, H, W)):
            raise ValueError(f"the generator's points must be {(n, 3, H, W)} or {(n, H, W, 3)} (the frames' size), got {tuple(extra.shape)}")
    elif engine == "moge":
        _lib.check_tensor("the generator's intrinsics", extra, torch.float32, (n, 3, 3))
    else:
        _lib.check_tensor("the generator's focallength_px", extra, (torch.float32, torch.float64), (n,))
    return depth, extra


def run_clip(args, color_video, infer):
    """u3d:132-191 / mge:124-177 / dpr:113-164 for one clip -> the depth video's path."""
    from metric_depth_video_toolbox_amd import depth_engines as host, step_clip
    da3_tool = sibling_tool("video_da3")
    engine = args.engine
    with step_clip.StepClip() as clip:
        color, = clip.open_checked([(color_video, "color_video", Exception("input color_video does not exist"))],       # u3d:132-133
                                   args.video_decoder, args.video_encoder, lambda n: host.frames_to_write(n, args.max_frames))
        n, H, W = clip.n, clip.H, clip.W
        tmp, final, xfov_file = host.engine_output_paths(color_video, clip.video)
        cam = host.requested_camera(args.xfov, args.yfov, W, H)
        if engine == "moge" and cam is not None:
            cam = np.float32(host.xfov_moge(cam))                                                       # mge:136: the model takes fov_x
        xfovs = []
        with clip.device(tmp, final) as (ctx, fetch, store):
            for a in range(0, n, int(args.batch)):
                b = min(n, a + int(args.batch))
                frames = model_frames(ctx, fetch(color, a, b), as_float=engine == "moge")
                depth, extra = checked_prediction(infer(frames, cam), engine, b - a, W, H)
                if engine == "unik3d":
                    focal = focal_from_points(ctx, extra).cpu().numpy()                                  # the batch's one read-back: 8 B per frame
                    xfovs += [host.xfov_unik3d(fx, fy, W, H) for fx, fy in focal]
                elif engine == "moge":
                    xfovs += [host.xfov_moge(K) for K in extra.cpu().numpy()]
                else:
                    xfovs += [host.xfov_depthpro(f, W, H) for f in extra.cpu().numpy()]
                store(da3_tool.depth_video_codes(ctx, depth, args.max_depth, (W, H), nan_to_max=engine == "moge"), a)
            # the x-fov list first, then the depth video's rename, as u3d:185-191 orders them: a depth video never stands without
            # its list, and a list that cannot be written leaves no depth video
            host.write_xfovs(xfov_file, xfovs)
    return final


def run(args, infer=None):
    """The step for --color_video, or for each entry of a .txt list.  infer: the generator (default: the one --generator names,
    loaded once).  -> the depth videos' paths."""
    from metric_depth_video_toolbox_amd import depth_engines as host, step_clip
    return step_clip.run_list(args, infer, host.check_engine_flags, lambda: host.load_generator(args.generator, args.engine), run_clip)


def main(argv=None):
    from metric_depth_video_toolbox_amd import depth_engines as host
    for path in run(host.build_engine_parser().parse_args(argv)):
        print(f"saved: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
