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

The three entry points of include/mdvt_depth_engines.h are bound in _lib.py and have no wrapper in the package yet (their tensor
contract records are the follow-up), so this tool hands the tensors over itself, as tools/video_da3.py does."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def sibling_tool(name):
    """tools/<name>.py as a module, loaded once."""
    key = "mdvt_tool_" + name
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(HERE, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[key] = mod
        spec.loader.exec_module(mod)
    return sys.modules[key]


def model_frames(ctx, frames, out_size=None, *, as_float=False, bgr=False, stream=None):
    """mdvt_model_frames on uint8 CUDA frames [N, H, W, 3] (rows and frames may be strided; B, G, R with bgr) -> the planar tensor
    [N, 3, h, w] in R, G, B plane order at out_size = (w, h) (default: the frames' own size), uint8, or float32 v / 255 with as_float.
    Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib, step_clip
    _lib.check_tensor("frames", frames, torch.uint8, (None, None, None, 3), packed=2, disjoint=True)
    N, H, W = step_clip.non_empty("frames", frames, "pixel")
    w, h = (W, H) if out_size is None else step_clip.size_arg(out_size, "out_size")
    dev = frames.device
    s = step_clip.stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, 3, h, w), dtype=torch.float32 if as_float else torch.uint8, device=dev)
    e = out.element_size()
    ctx.call("mdvt_model_frames", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), int(bool(bgr)), w, h, int(bool(as_float)),
             out.data_ptr(), e * w, e * w * h, e * w * h * 3, _lib.stream_arg(dev, s))
    return out


def depth_prompt(ctx, codes, max_depth, out_size, *, bgr=False, stream=None):
    """mdvt_depth_prompt on uint8 CUDA depth frames [N, H, W, 3] (R, G, B; B, G, R with bgr) -> float32 [N, h, w] at out_size = (w, h):
    the decoded depth, resized like cv2.resize(INTER_LINEAR).  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib, step_clip
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    _lib.check_tensor("codes", codes, torch.uint8, (None, None, None, 3), packed=2, disjoint=True)
    N, H, W = step_clip.non_empty("codes", codes, "pixel")
    w, h = step_clip.size_arg(out_size, "out_size")
    dev = codes.device
    s = step_clip.stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        out = torch.empty((N, h, w), dtype=torch.float32, device=dev)
    ctx.call("mdvt_depth_prompt", W, H, N, codes.data_ptr(), codes.stride(1), codes.stride(0), int(bool(bgr)), float(max_depth), w, h,
             out.data_ptr(), 4 * w, 4 * w * h, _lib.stream_arg(dev, s))
    return out


def focal_from_points(ctx, points, *, want_counts=False, stream=None):
    """mdvt_focal_from_points on float32 CUDA point maps [N, H, W, 3] or [N, 3, H, W] (a last dimension of 3 is read as the
    former, as u3d:46-52 reads it; rows, planes and frames may be strided) -> float32 [N, 2] = (fx, fy) per frame and, with
    want_counts, the int32 tensor [N, 2] = (nx, ny) of the library's uint32 counts (at most 2^28 each).  Only enqueues, on `stream`."""
    import torch
    from metric_depth_video_toolbox_amd import _lib, step_clip
    _lib.check_tensor("points", points, torch.float32, ndim=4)
    if points.shape[-1] == 3:
        _lib.check_tensor("points", points, torch.float32, ndim=4, packed=2, disjoint=True)
        layout, dims = 1, points.shape[:3]
        pitch, plane, stride = 4 * points.stride(1), 0, 4 * points.stride(0)
    elif points.shape[1] == 3:
        _lib.check_tensor("points", points, torch.float32, ndim=4, packed=1, disjoint=True)
        layout, dims = 0, (points.shape[0], *points.shape[2:])
        pitch, plane, stride = 4 * points.stride(2), 4 * points.stride(1), 4 * points.stride(0)
    else:
        raise ValueError(f"points must be [N, H, W, 3] or [N, 3, H, W], got shape {tuple(points.shape)}")
    N, H, W = step_clip.non_empty("points", points, "point", dims)
    dev = points.device
    s = step_clip.stream_or_current(dev, stream)
    with torch.cuda.stream(s):
        focal = torch.empty((N, 2), dtype=torch.float32, device=dev)
        counts = torch.empty((N, 2), dtype=torch.int32, device=dev) if want_counts else None
    ctx.call("mdvt_focal_from_points", W, H, N, points.data_ptr(), layout, pitch, plane, stride, focal.data_ptr(),
             counts.data_ptr() if want_counts else None, _lib.stream_arg(dev, s))
    return (focal, counts) if want_counts else focal


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
