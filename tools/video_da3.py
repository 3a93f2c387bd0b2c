#!/usr/bin/env python3
"""The reference's video_da3.py (vd3:) around its model, on the device: the depth step movie_2_3D.py picks when no engine is named.

    python tools/video_da3.py --color_video x.mkv [--max_frames N --max_depth 100 --images_per_batch 40 --batch_overlap 6
           --nr_of_ref_frames 6 --da3_resolution 504 --video_decoder host|device|device_all --video_encoder host|device]
           --generator pkg.module:callable

writes x.mkv_depth.mkv (tmp x.mkv_tmp_depth.mkv, then verify_and_move), x.mkv_depth.mkv_xfovs.json and
x.mkv_depth.mkv_transformations.json, the three files the render takes.  A .txt list runs each entry; a .npy frame dump gives .npy
depth frames.  INTEGRATION.md states the generator's contract.

The schedule, the pose alignment, the parser and the file names are host logic in metric_depth_video_toolbox_amd/video_da3.py; the
opening of the clip with its checks, the context, the output file and the list loop are step_clip.py's, shared with the other model
steps.  Here is what touches the device: the frames are gathered there (the reference frames are decoded once and kept), the model is called, the
factor that aligns a batch to the one before comes from the fit's float32 sums (video_metric_convert.compute_scale_and_shift_full)
and stays on the device, and the new planes go through mdvt_depth_video_codes (include/mdvt_depth_sink.h) with that factor to the
video's size and on to the writer or the device FFV1 encoder.  One 4-byte read-back of the factor per batch scales the translations
(vd3:192).  depth_video_codes, the wrapper of mdvt_depth_video_codes, is metric_depth_video_toolbox_amd/step_device.py's; it stays
reachable under this module's name.

save_depth_video below is the sink alone (dfh:125-161), for any metric model's float32 CUDA planes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from metric_depth_video_toolbox_amd.step_device import depth_video_codes      # noqa: E402


def batch_scale(earlier, again):
    """The factor s with earlier ~ s * again over float32 CUDA planes [N, h, w] of the same frames, as a one-element float32 CUDA
    tensor: fl(sum(earlier * again) / max(sum(again * again), 1e-12)).  The two float32 sums are b_0 and a_00 of the fit with
    prediction `again` and target `earlier` (NumPy's order of summation).  The quotient is taken in float64 and rounded once more: for
    two float32 operands that is the correctly rounded float32 quotient, whatever the device's float32 division does.  No read-back."""
    import torch
    from metric_depth_video_toolbox_amd import video_metric_convert as vmc
    v = vmc.compute_scale_and_shift_full(again, earlier).values
    return (v[3:4].double() / torch.clamp_min(v[0:1], 1e-12).double()).float()      # (the floor in float32; a NaN sum stays NaN)


def checked_prediction(got, T):
    """What a generator returned -> (depth float32 CUDA [T, h, w], extrinsics host [T, 3, 4], intrinsics host [T, 3, 3]), or the
    TypeError / ValueError of the contract, before anything is launched on it."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    if not isinstance(got, (tuple, list)) or len(got) != 3:
        raise TypeError("the generator must return (depth, extrinsics, intrinsics)")
    depth, ext, intr = got
    _lib.check_tensor("the generator's depth", depth, torch.float32, (T, None, None), packed=1, disjoint=True)
    if depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"the generator's depth holds no value: shape {tuple(depth.shape)}")
    host = []
    for name, m, shape in (("extrinsics", ext, (T, 3, 4)), ("intrinsics", intr, (T, 3, 3))):
        m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
        if m.dtype.kind != "f":
            raise TypeError(f"the generator's {name} must have a float dtype, got {m.dtype}")
        if tuple(m.shape) != shape:
            raise ValueError(f"the generator's {name} must be {shape}, got {tuple(m.shape)}")
        host.append(m)
    return depth, host[0], host[1]


def save_depth_video(frames, path, fps, max_depth, W, H, *, nan_to_max=False, video_encoder="host", batch=16):
    """dfh:125-161 for float32 CUDA planes [N, h, w] of metric depth from any model: resized to W x H, coded and written to `path`
    (an .mkv at `fps`; a .npy dump of the coded frames with fps None).  nan_to_max: moge_video.py:171's rule in front."""
    import torch
    from metric_depth_video_toolbox_amd import _lib
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput, check_video_encoder
    check_video_encoder(video_encoder, fps is not None)
    _lib.check_tensor("frames", frames, torch.float32, ndim=3, packed=1, disjoint=True)
    n, dev = int(frames.shape[0]), frames.device
    ctx = _lib.Context(_lib.device_index(dev), 16, 16)
    try:
        with torch.cuda.device(dev), ClipOutput(path, path, n, (int(H), int(W), 3), fps, video_encoder, ctx) as out:
            for a in range(0, n, max(1, int(batch))):
                out.store(depth_video_codes(ctx, frames[a:a + max(1, int(batch))], max_depth, (W, H), nan_to_max=nan_to_max), a)
    finally:
        ctx.close()
    return path


def run_clip(args, color_video, infer):
    """vd3:68-263 for one clip -> the depth video's path."""
    import torch
    from metric_depth_video_toolbox_amd import step_clip, video_da3 as host
    with step_clip.StepClip() as clip:
        color, = clip.open_checked([(color_video, "color_video", Exception("video file: " + color_video + " does not exist"))],     # dfh:257-258
                                   args.video_decoder, args.video_encoder,
                                   lambda n: min(n, args.max_frames) if args.max_frames > 0 else n)                             # dfh:273
        schedule = host.batch_schedule(clip.n, args.images_per_batch, args.batch_overlap, args.nr_of_ref_frames)
        tmp, final, xfov_file, transformations_file = host.output_paths(color_video, clip.video)
        with clip.device(tmp, final) as (ctx, fetch, store):
            n_refs = schedule[0][1]
            ref_frames = [fetch(color, i, i + 1) for i in schedule[0][0][:n_refs]]               # decoded once, kept
            poses = host.PoseTrack(args.batch_overlap)
            first_ref_depths = last_frames = last_depths = None
            at = 0
            for ids, used in schedule:
                n_new = len(ids) - used
                new_frames = fetch(color, ids[used], ids[-1] + 1)
                frames = torch.cat(ref_frames + ([last_frames] if last_frames is not None else []) + [new_frames])
                depth, ext, intr = checked_prediction(infer(frames, args.da3_resolution), len(ids))
                if first_ref_depths is None:
                    first_ref_depths = depth[:used].clone()                                     # vd3:178-179
                scale = None
                if last_depths is not None:                                                     # vd3:183-193
                    scale = batch_scale(torch.cat([first_ref_depths, last_depths]), depth[:used])
                store(depth_video_codes(ctx, depth[used:], args.max_depth, (clip.W, clip.H), scale=scale), at)
                at += n_new
                handed = len(ids[used:][-args.batch_overlap:])              # the frames the next batch sees again (vd3:239-241)
                last_frames = new_frames[-handed:]
                last_depths = depth[-handed:] if scale is None else depth[-handed:] * scale
                poses.add(ext, intr, used, None if scale is None else float(scale.item()))      # the batch's one read-back (vd3:192)
    host.write_json_files(xfov_file, transformations_file, poses.xfovs(), poses.transformations())
    return final


def run(args, infer=None):
    """The step for --color_video, or for each entry of a .txt list.  infer: the generator (default: the one --generator names,
    loaded once).  -> the depth videos' paths."""
    from metric_depth_video_toolbox_amd import step_clip, video_da3 as host

    def check(a):                                                   # before any file is opened
        host.check_flags(a)
        host.check_schedule_args(a.images_per_batch, a.batch_overlap, a.nr_of_ref_frames)
    return step_clip.run_list(args, infer, check, lambda: host.load_generator(args.generator), run_clip)


def main(argv=None):
    from metric_depth_video_toolbox_amd import video_da3 as host
    for path in run(host.build_parser().parse_args(argv)):
        print(f"saved: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
