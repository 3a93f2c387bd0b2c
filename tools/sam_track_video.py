#!/usr/bin/env python3
"""The reference's depth-assisted camera-tracking step (sam_track_video.py, stv:) around MegaSAM's DROID tracker, on the device: a
colour video, its depth video and an optional mask video to the camera poses every `--transformation_file` consumer reads.

    python tools/sam_track_video.py --color_video x.mkv --depth_video x.mkv_depth.mkv --xfov F|--yfov F [--mask_video m.mkv
           --max_frames N --max_depth 100 --optimize_intrinsic --batch 8 --video_decoder host|device|device_all
           --video_encoder host|device] --generator pkg.module:callable

writes x.mkv_depth.mkv_transformations.json, x.mkv_depth.mkv_megasam.mkv (the tracker's depth) and x.mkv_depth.mkv_megasam_motion.mkv
(its motion probability), each under a temporary name first; the videos are renamed when their frame count is right.  .npy frame
dumps give .npy frames.  INTEGRATION.md states the tracker's contract.

The parser, the file names, the tracker's size, the intrinsics, the frames the reference's look-ahead loop hands over (frame_plan) and
the pose conversion are host logic in metric_depth_video_toolbox_amd/sam_track.py; the opening of the clip with its checks, the
context and the outputs are step_clip.py's and clip_io.py's.  Here is what touches the device.  Each decoded batch goes through
mdvt_area_model_frames, mdvt_tracker_depth and mdvt_tracker_mask (metric_depth_video_toolbox_amd/megasam_device.py) and is handed to the tracker frame by
frame as views; after the tracker's global alignment its depth and motion planes go through mdvt_tracker_outputs to the writer or the
device FFV1 encoder.  The frames stay on the device from decoder to writer; the clip's one read-back is the poses and the first
frame's intrinsics."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metric_depth_video_toolbox_amd.megasam_device import area_model_frames, tracker_depth, tracker_mask, tracker_outputs      # noqa: E402


def checked_results(got):
    """What tracker.terminate returned -> (traj [t, 7], depth [t, h, w], motion [t, h, w], intrinsics [>= 1, 4]) as float32 CUDA
    tensors, or the TypeError / ValueError of the contract, before anything is launched on them."""
    import torch
    if not isinstance(got, (tuple, list)) or len(got) != 4:
        raise TypeError("tracker.terminate must return (traj_est, depth_est, motion_prob, intrinsics)")
    for name, t in zip(("traj_est", "depth_est", "motion_prob", "intrinsics"), got):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_floating_point():
            raise TypeError(f"the tracker's {name} must be a floating-point CUDA tensor")
    traj, depth, motion, intr = (t.to(torch.float32) for t in got)
    if traj.ndim != 2 or traj.shape[1] != 7 or traj.shape[0] < 1:
        raise ValueError(f"the tracker's traj_est must be [t, 7] with t >= 1, got {tuple(traj.shape)}")
    t = traj.shape[0]
    for name, p in (("depth_est", depth), ("motion_prob", motion)):
        if p.ndim != 3 or p.shape[0] != t or min(p.shape) < 1:
            raise ValueError(f"the tracker's {name} must be [{t}, h, w], got {tuple(p.shape)}")
    if intr.ndim != 2 or intr.shape[0] < 1 or intr.shape[1] != 4:
        raise ValueError(f"the tracker's intrinsics must be [>= 1, 4], got {tuple(intr.shape)}")
    return traj, depth, motion, intr


def run_clip(args, make_tracker):
    """stv:43-245 for one clip -> {"json", "depth", "motion"}: the written paths."""
    import torch
    from metric_depth_video_toolbox_amd import sam_track as host, step_clip
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    with step_clip.StepClip() as clip:
        inputs = [(args.depth_video, "depth_video", Exception("input depth_video does not exist")),       # stv:51-52; its size and rate rule (stv:56-58)
                  (args.color_video, "color_video", Exception("input color_video does not exist"))]       # stv:48-49
        if args.mask_video is not None:
            inputs.append((args.mask_video, "mask_video", Exception("input mask_video does not exist")))   # stv:64-65
        opened = clip.open_checked(inputs, args.video_decoder, args.video_encoder, lambda n: n, label="--{name}")
        depth, color, mask = opened[0], opened[1], (opened[2] if len(opened) > 2 else None)
        H, W = clip.H, clip.W
        for (_, name, _), f in zip(inputs[1:], opened[1:]):
            if (int(f.shape[1]), int(f.shape[2])) != (H, W):
                raise ValueError(f"--{name} is {int(f.shape[2])} x {int(f.shape[1])}, the depth video {W} x {H}: the videos must have one size")
        count, final_index = host.frame_plan(len(depth), len(color), None if mask is None else len(mask), args.max_frames)
        if count < 1:
            raise ValueError("No frames read")
        h1, w1, hc, wc = host.model_size(H, W)
        if hc < 8 or wc < 8:
            raise ValueError(f"{W} x {H} frames give the tracker an image of {wc} x {hc}")
        paths = host.output_paths(args.depth_video, clip.video)
        k = host.scaled_intrinsics(host.camera_matrix(args.xfov, args.yfov, W, H), H, W, h1, w1)
        batch = int(args.batch)
        clip.on_device(torch.device("cuda", torch.cuda.current_device()), *clip.codecs, own_context=True)
        with torch.cuda.device(clip.dev):
            ctx, dev = clip.ctx, clip.dev
            intr = torch.from_numpy(k).to(dev)
            tracker = make_tracker([hc, wc])                                                        # stv:169-189
            stream = []
            for a in range(0, count, batch):
                b = min(count, a + batch)
                images = area_model_frames(ctx, clip.fetch(color, a, b), (w1, h1), (wc, hc))        # stv:143-148
                depths = tracker_depth(ctx, clip.fetch(depth, a, b), args.max_depth, (w1, h1), (wc, hc))     # stv:125-131, 150-154
                masks = tracker_mask(ctx, clip.fetch(mask, a, b), (w1, h1), (wc, hc)) if mask is not None else torch.ones_like(depths)
                for i in range(a, b):
                    item = (i, images[i - a:i - a + 1], depths[i - a], intr.clone(), masks[i - a])  # stv:191
                    stream.append(item)
                    if i == final_index:
                        tracker.track_final(*item)
                    else:
                        tracker.track(*item)
            print("Do global alignment")
            traj, depth_est, motion, est_intr = checked_results(tracker.terminate(stream, bool(args.optimize_intrinsic)))
            t = int(traj.shape[0])
            for what, planes, mode, top in (("depth", depth_est, 0, float(args.max_depth)), ("motion", motion, 1, 1.0)):     # stv:222-234
                tmp, final = paths[what]
                with ClipOutput(tmp, final, t, (H, W, 3), clip.fps, clip.codecs[1], ctx) as out:
                    for a in range(0, t, batch):
                        out.store(tracker_outputs(ctx, planes[a:a + batch], mode, top, (W, H)), a)
            back = torch.cat([traj.reshape(-1), est_intr[0].reshape(-1)]).cpu().numpy()             # the clip's one read-back
        host.write_transformations(*paths["json"], host.poses_to_transformations(back[:7 * t].reshape(t, 7)))
        fovx, fovy = host.estimated_fov(back[7 * t:])
        print("Estimated intrinsics:", "fovx:", fovx, "fovy", fovy)
    return {what: final for what, (_, final) in paths.items()}


def run(args, make_tracker=None):
    """The step for one clip.  make_tracker: the tracker's factory (default: the one --generator names)."""
    from metric_depth_video_toolbox_amd import sam_track as host
    host.check_flags(args)                                          # before any file is opened
    if make_tracker is None:
        make_tracker = host.load_generator(args.generator)
    return run_clip(args, make_tracker)


def main(argv=None):
    from metric_depth_video_toolbox_amd import sam_track as host
    for what, path in run(host.build_parser().parse_args(argv)).items():
        print(f"saved: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
