#!/usr/bin/env python3
"""The reference's MVSAnywhere depth step (video_mvsa.py, mvs:) around its model, on the device: a colour video and its camera poses
(the transformations the Depth-Anything-3 step writes) to the multi-view metric depth video x.mkv_depth.mkv that the render reads.

    python tools/video_mvsa.py --color_video x.mkv|list.txt --xfov F|--yfov F [--transformation_file t.json --max_frames N --window 7
           --resize_w 1024 --fast_cost_volume --max_depth 100 --apply_cost_volume_scale --save_cost_volume_scales --batch 8
           --video_decoder host|device|device_all --video_encoder host|device] --generator pkg.module:callable

writes x.mkv_depth.mkv (tmp x.mkv_tmp_depth.mkv, renamed when its frame count is right) and, with --save_cost_volume_scales,
x.mkv_depth.mkv_cv_scales.json.  A .txt list runs each entry; a .npy frame dump gives .npy depth frames.  INTEGRATION.md states the
generator's contract.

The parser, the transformation file's three forms, the window, the sizes and the intrinsics are host logic in
metric_depth_video_toolbox_amd/video_mvsa.py; the opening of the clip with its checks, the context, the output file and the list loop
are step_clip.py's.  Here is what touches the device.  Each decoded batch goes ONCE through
mdvt_bilinear_model_frames into a ring of 2 * half_w + 1 + batch planar frames (the reference resizes a frame again for every window
it falls into, up to `window` times, on the CPU); per target frame the two dicts of mvs:171-231 are built from views of the ring, the
model is called, and its refined depth goes through mdvt_nearest_depth_codes to the writer or the device FFV1 encoder.

--apply_cost_volume_scale (off by default, which is the reference's behaviour) runs mdvt_ratio_median and hands its device float to
the codes as their factor, with no read-back: the `* s` that mvs:297 comments out.  It is THIS PROJECT'S READING of the author's
intent ("Not sure if this is right rescaling", mvs:259), not the reference's output.  --save_cost_volume_scales reads the clip's
medians back once, at its end.

bilinear_model_frames, nearest_depth_codes and ratio_median, the wrappers of include/mdvt_mvsa.h's three entry points, are
metric_depth_video_toolbox_amd/step_device.py's; they stay reachable under this module's name."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metric_depth_video_toolbox_amd.step_device import bilinear_model_frames, nearest_depth_codes, ratio_median      # noqa: E402


def checked_prediction(got):
    """What a generator returned -> (depth float32 CUDA [1, h_ref, w_ref], lowest cost float32 CUDA [1, h_cv, w_cv], mask uint8 CUDA
    [1, h_m, w_m] or None), or the TypeError / ValueError of the contract, before anything is launched on it."""
    import torch
    if not isinstance(got, dict) or "depth_pred_s0_b1hw" not in got or "lowest_cost_bhw" not in got:
        raise TypeError("the generator must return a dict with 'depth_pred_s0_b1hw' and 'lowest_cost_bhw'")
    depth, cv = got["depth_pred_s0_b1hw"], got["lowest_cost_bhw"]
    for name, t, ndim in (("depth_pred_s0_b1hw", depth, 4), ("lowest_cost_bhw", cv, 3)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_floating_point():
            raise TypeError(f"the generator's {name} must be a floating-point CUDA tensor")
        if t.ndim != ndim or t.shape[0] != 1 or (ndim == 4 and t.shape[1] != 1) or min(t.shape) < 1:
            raise ValueError(f"the generator's {name} must be [1, {'1, ' if ndim == 4 else ''}h, w], got {tuple(t.shape)}")
    mask = None
    if "overall_mask_bhw" in got:                                   # mvs:271-276
        mask = got["overall_mask_bhw"]
    elif "overall_mask_b1hw" in got:
        mask = got["overall_mask_b1hw"]
        if isinstance(mask, torch.Tensor) and mask.ndim == 4:
            mask = mask[:, 0]
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.ndim != 3 or mask.shape[0] != 1 or min(mask.shape) < 1:
            raise ValueError("the generator's mask must be a CUDA tensor [1, h, w] (overall_mask_bhw) or [1, 1, h, w] (overall_mask_b1hw)")
        mask = mask.to(torch.bool).to(torch.uint8).contiguous()
    return depth[:, 0].to(torch.float32).contiguous(), cv.to(torch.float32).contiguous(), mask      # mvs:261-262


def run_clip(args, color_video, infer):
    """mvs:81-307 for one clip -> the depth video's path."""
    import torch
    from metric_depth_video_toolbox_amd import step_clip, video_mvsa as host
    with step_clip.StepClip() as clip:
        color, = clip.open_checked([(color_video, "color_video", Exception("input video missing"))],   # mvs:81
                                   args.video_decoder, args.video_encoder, lambda n: host.frames_to_read(n, args.max_frames))
        n, H, W = clip.n, clip.H, clip.W
        tmp, final, scales_file = host.output_paths(color_video, clip.video)
        new_w, new_h, _ = host.model_size(W, H, args.resize_w)
        if new_w < 1 or new_h < 1:
            raise ValueError(f"--resize_w {args.resize_w} gives a model size of {new_w} x {new_h} for {W} x {H} frames")
        K44, invK44, K44_s, invK44_s = host.intrinsics(args.xfov, args.yfov, W, H, args.resize_w)
        cam_T_world = torch.from_numpy(host.load_transforms(args.transformation_file, n))               # [n, 4, 4] float32 (mvs:110)
        world_T_cam = torch.stack([torch.inverse(cam_T_world[i]) for i in range(n)])                    # mvs:168-169, on the CPU
        half, batch = host.half_window(args.window), int(args.batch)
        want_scales = bool(args.apply_cost_volume_scale or args.save_cost_volume_scales)
        with clip.device(tmp, final) as (ctx, fetch, store):
            dev = clip.dev
            cap = 2 * half + 1 + batch
            ring = torch.empty((cap, 3, new_h, new_w), dtype=torch.float32, device=dev)
            cam_T_world, world_T_cam = cam_T_world.to(dev), world_T_cam.to(dev)
            Kd, iKd, Ksd, iKsd = (t.unsqueeze(0).to(dev) for t in (K44, invK44, K44_s, invK44_s))  # [1, 4, 4] each
            full_res = torch.zeros(1, 1, H, W, device=dev)                                          # mvs:191, allocated once
            scales = torch.ones((n,), dtype=torch.float32, device=dev) if want_scales else None
            loaded = 0
            codes, first = None, 0
            for i in range(n):
                while loaded < min(n, i + half + 1):                                                # the frames the window needs
                    b = min(n, loaded + batch)
                    frames = fetch(color, loaded, b)
                    at = loaded % cap
                    k = min(b - loaded, cap - at)                                                   # the ring's end splits a batch
                    bilinear_model_frames(ctx, frames[:k], (new_w, new_h), out=ring[at:at + k])
                    if k < b - loaded:
                        bilinear_model_frames(ctx, frames[k:], (new_w, new_h), out=ring[:b - loaded - k])
                    loaded = b
                ref_idx = host.reference_indices(i, n, args.window)
                R = len(ref_idx)
                cur_data = {                                                                        # mvs:171-192
                    "image_b3hw": ring[i % cap].unsqueeze(0),
                    "K_s0_b44": Ksd, "invK_s0_b44": iKsd, "K_matching_b44": Ksd, "invK_matching_b44": iKsd,
                    "K_full_depth_b44": Kd, "invK_full_depth_b44": iKd,
                    "cam_T_world_b44": cam_T_world[i].unsqueeze(0), "world_T_cam_b44": world_T_cam[i].unsqueeze(0),
                    "frame_id_string": [f"{i:06d}"],
                    "full_res_depth_b1hw": full_res,
                }
                src_T_cw = cam_T_world[ref_idx]                                                     # [R, 4, 4]
                src_data = {                                                                        # mvs:218-231
                    "image_b3hw": torch.stack([ring[j % cap] for j in ref_idx]).unsqueeze(0),
                    "K_s0_b44": Ksd.expand(R, 4, 4).unsqueeze(0), "invK_s0_b44": iKsd.expand(R, 4, 4).unsqueeze(0),
                    "K_matching_b44": Ksd.expand(R, 4, 4).unsqueeze(0), "invK_matching_b44": iKsd.expand(R, 4, 4).unsqueeze(0),
                    "K_full_depth_b44": Kd.expand(R, 4, 4).contiguous().unsqueeze(0),
                    "invK_full_depth_b44": iKd.expand(R, 4, 4).contiguous().unsqueeze(0),
                    "cam_T_world_b44": src_T_cw.unsqueeze(0), "world_T_cam_b44": torch.inverse(src_T_cw).unsqueeze(0),     # mvs:215
                    "frame_id_string": [f"{j:06d}" for j in ref_idx],
                }
                depth, cv, mask = checked_prediction(infer(cur_data, src_data, bool(args.fast_cost_volume)))
                if want_scales:
                    ratio_median(ctx, cv, depth, mask, out=scales[i:i + 1])                         # mvs:283-293, kept on the device
                if codes is None:
                    first, codes = i, torch.empty((min(batch, n - i), H, W, 3), dtype=torch.uint8, device=dev)
                nearest_depth_codes(ctx, depth, (cv.shape[2], cv.shape[1]), args.max_depth, (W, H),
                                    scale=scales[i:i + 1] if args.apply_cost_volume_scale else None, out=codes[i - first:i - first + 1])
                if i - first + 1 == codes.shape[0]:
                    store(codes, first)
                    codes = None
            if args.save_cost_volume_scales:
                host.write_scales(scales_file, scales.cpu().numpy())                                # the clip's one read-back
    return final


def run(args, infer=None):
    """The step for --color_video, or for each entry of a .txt list.  infer: the generator (default: the one --generator names,
    loaded once).  -> the depth videos' paths."""
    from metric_depth_video_toolbox_amd import step_clip, video_mvsa as host

    def check(a):                                                   # before any file is opened for writing
        host.check_flags(a)
        host.check_transformation_file(a.transformation_file)
    return step_clip.run_list(args, infer, check, lambda: host.load_generator(args.generator), run_clip)


def main(argv=None):
    from metric_depth_video_toolbox_amd import video_mvsa as host
    for path in run(host.build_parser().parse_args(argv)):
        print(f"saved: {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
