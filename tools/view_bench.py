#!/usr/bin/env python3
"""Times the free-camera viewer's centres (view_depthfile.centers, mdvt_view_centers) on the synthetic track at 1080p and at
3840 x 2160, mesh and points with parked vertices, 8 posed frames per call, and records how far NumPy's order of summation -- the
device's -- lies from the sequential order of Open3D's get_center on that content.

    python tools/view_bench.py [--frames 8] [--repeats 5] [--calls 500] [--out FILE]

Per case: `repeats` timed windows of `calls` calls each (0.1 to 0.4 s a window at the defaults) after a warm-up window, every window
ended by a device synchronise; the median window, the spread (max - min over the median) and the rate in frames/s.  The order difference is computed on the host in
f64 (np.cumsum adds in sequence) from the reference vertices of tests/view_ref.py for the case's first frame, next to the bound
of include/mdvt_view.h.  Prints one JSON line per case; --out also writes them to a file.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_bench needs a GPU")
    import view_ref as vr
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    from metric_depth_video_toolbox_amd.stereo_rerender import StereoRerenderer
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene, synthetic_pose_track

    lines = []
    for W, H in ((1920, 1080), (3840, 2160)):
        scene = SyntheticScene(W, H, config_id=4)
        depth = np.stack([scene.frame(k)[0] for k in range(args.frames)])
        track = synthetic_pose_track(args.frames)
        d = torch.from_numpy(depth).cuda()
        for mode, kw in (("mesh", {}), ("points_parked", dict(render_as_pointcloud=True, remove_edges=True))):
            r = StereoRerenderer(W, H, device=0, **kw)
            params = r.pack_params([r.frame_params(xfov=45.0, transformation=np.asarray(track[k]).reshape(4, 4)) for k in range(args.frames)],
                                   args.frames)
            windows = []
            for rep in range(args.repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    got = vd.centers(d, params, r)
                torch.cuda.synchronize()
                if rep:
                    windows.append((time.perf_counter() - t0) / args.calls)
            med = float(np.median(windows))
            K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
            P = vr.vertices(depth[0], K, mesh=mode == "mesh", remove_edges=mode != "mesh", T=np.asarray(track[0]).reshape(4, 4),
                            depth_scale=params[0].depth_scale)
            want = vr.center_of(P)
            seq = np.array([np.cumsum(np.ascontiguousarray(P[:, c]))[-1] / P.shape[0] for c in range(3)])
            line = dict(what="view_centers", size=f"{W}x{H}", mode=mode, frames=args.frames, ms_per_call=med * 1e3,
                        spread=float((max(windows) - min(windows)) / med), frames_per_s=args.frames / med,
                        device_equals_numpy_order=bool(got[0].cpu().numpy().tobytes() == want.tobytes()),
                        order_difference=[float(v) for v in np.abs(want - seq)], bound=[float(v) for v in vr.center_bound(P)])
            print(json.dumps(line), flush=True)
            lines.append(line)
            r.close()
    # the view render against the only way to get its image without it: the stereo posed render with ipd_m = 0 and the same composed
    # matrices.  The two alternate window by window; the spread is each one's own.
    for W, H in ((1920, 1080), (3840, 2160)):
        scene = SyntheticScene(W, H, config_id=4)
        fr = [scene.frame(k) for k in range(args.frames)]
        d = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
        c = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
        track = synthetic_pose_track(args.frames)
        for mode, pc in (("mesh", False), ("points", True)):
            r = vd.view_renderer(W, H, device=0, render_as_pointcloud=pc)
            params = [r.frame_params(xfov=45.0, transformation=np.asarray(track[k]).reshape(4, 4)) for k in range(args.frames)]
            cen = vd.centers(d, params, r).cpu().numpy()
            cam = vd.camera_position(0.2 * cen[0, 2], 0.2 * cen[0, 2], -0.4 * cen[0, 2])
            views = np.stack([vd.look_at_view(cam, cen[k]) for k in range(args.frames)])
            vp = vd.view_params(params, views)
            sbs = torch.empty((args.frames, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
            smask = torch.empty((args.frames, H, 2 * W), dtype=torch.uint8, device="cuda")
            calls = max(4, args.calls // 25)
            run = {"view": lambda: vd.render_view(d, c, views, params, r), "stereo_ipd0": lambda: r.render(d, c, vp, out_sbs=sbs, out_mask=smask)}
            windows = {"view": [], "stereo_ipd0": []}
            for rep in range(args.repeats + 1):
                for name, fn in run.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        fn()
                    torch.cuda.synchronize()
                    if rep:
                        windows[name].append((time.perf_counter() - t0) / calls)
            mv, ms = float(np.median(windows["view"])), float(np.median(windows["stereo_ipd0"]))
            line = dict(what="view_render", size=f"{W}x{H}", mode=mode, frames=args.frames, calls_per_window=calls,
                        view_ms=mv * 1e3, view_spread=float((max(windows["view"]) - min(windows["view"])) / mv),
                        stereo_ipd0_ms=ms * 1e3, stereo_spread=float((max(windows["stereo_ipd0"]) - min(windows["stereo_ipd0"])) / ms),
                        stereo_over_view=ms / mv, slowest_view_over_fastest_stereo=max(windows["view"]) / min(windows["stereo_ipd0"]))
            print(json.dumps(line), flush=True)
            lines.append(line)
            r.close()
    if args.out:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
