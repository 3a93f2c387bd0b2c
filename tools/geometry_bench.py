#!/usr/bin/env python3
"""Times the geometry export (mdvt_export_geometry_batch, include/mdvt_geometry.h) on the synthetic track at 1080p: 8 frames a call,
remove_edges on and off, each output set on its own and all together, and the grey depth; next to it the NumPy and oracle
restatement of tests/geometry_ref.py for one frame, timed on the same box's CPU.

    python tools/geometry_bench.py [--frames 8] [--batches 4] [--repeats 5] [--calls 40] [--sets all,...] [--out FILE]

Per case: `repeats` timed windows of `calls` calls each after a warm-up window, a pair of device events around every window; the
calls of a window cycle through `batches` distinct batches of frames (the lists of one batch do not stay in a cache for the next
call).  Reported: the median window as time per frame, the spread (max - min over the median), and the achieved bytes/s against the
algorithmic traffic -- inputs read once (3 N bytes of depth, 3 N of colour where point_rgb is asked for), outputs written once
(24 N of vertices, 12 M of triangles, 4 U + 24 U + 3 U of the vertex lists, 8 of counts) with U and M as the call counted them.
Prints one JSON line per case; --out also writes them to a file.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SETS = {"counts": (), "vertices": ("vertices",), "triangles": ("triangles",), "used_index": ("used_index",),
        "ply": ("points", "point_rgb"), "obj": ("vertices", "triangles"), "all": ("vertices", "triangles", "used_index", "points", "point_rgb")}
ITEM = {"vertices": 24, "triangles": 12, "used_index": 4, "points": 24, "point_rgb": 3}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--sets", type=str, default=",".join(SETS))
    ap.add_argument("--size", type=str, default="1920x1080")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geometry_bench needs a GPU")
    import geometry_ref as gr
    from metric_depth_video_toolbox_amd import _lib, depth_map_tools
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene, synthetic_pose_track

    W, H = (int(v) for v in args.size.split("x"))
    F, B = args.frames, args.batches
    N, ncell = W * H, (W - 1) * (H - 1)
    scene = SyntheticScene(W, H, config_id=4)
    fr = [scene.frame(k) for k in range(F * B)]
    depth = [torch.from_numpy(np.stack([f[0] for f in fr[b * F:(b + 1) * F]])).cuda() for b in range(B)]
    color = [torch.from_numpy(np.stack([f[1] for f in fr[b * F:(b + 1) * F]])).cuda() for b in range(B)]
    track = synthetic_pose_track(F * B)
    K = depth_map_tools.compute_camera_matrix(45.0, None, W, H)
    params = []
    for b in range(B):
        arr = (_lib.MdvtFrameParams * F)()
        for k in range(F):
            for i, v in enumerate(np.asarray(K, np.float64).reshape(9)):
                arr[k].K[i] = arr[k].Krender[i] = v
            arr[k].depth_scale, arr[k].has_T = 1.0, 1
            for i, v in enumerate(np.asarray(track[b * F + k], np.float64).reshape(16)):
                arr[k].T[i] = v
        params.append(arr)
    ctx = _lib.Context(0, W, H)
    stream = _lib.stream_arg(depth[0].device)
    bufs = {"vertices": torch.empty((F, N, 3), dtype=torch.float64, device="cuda"), "triangles": torch.empty((F, 2 * ncell, 3), dtype=torch.int32, device="cuda"),
            "used_index": torch.empty((F, N), dtype=torch.int32, device="cuda"), "points": torch.empty((F, N, 3), dtype=torch.float64, device="cuda"),
            "point_rgb": torch.empty((F, N, 3), dtype=torch.uint8, device="cuda")}
    counts = torch.zeros((F, 2), dtype=torch.int32, device="cuda")
    lines = []

    def timed(call):
        windows = []
        for rep in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.calls):
                call(k % B)
            e1.record()
            e1.synchronize()
            if rep:
                windows.append(e0.elapsed_time(e1) * 1e-3 / args.calls)
        med = float(np.median(windows))
        return med, float((max(windows) - min(windows)) / med)

    for remove in (1, 0):
        for name in args.sets.split(","):
            want = SETS[name]
            opts = _lib.MdvtGeometryOpts(decode=0, remove_edges=remove, max_depth=100.0)
            ios = []
            for b in range(B):
                io = _lib.MdvtGeometryIO()
                io.depth_rgb, io.depth_pitch, io.depth_stride = depth[b].data_ptr(), 3 * W, 3 * N
                io.color_rgb, io.color_pitch, io.color_stride = color[b].data_ptr(), 3 * W, 3 * N
                for n in want:
                    setattr(io, n, bufs[n].data_ptr())
                    setattr(io, {"used_index": "used_stride"}.get(n, n + "_stride"), bufs[n].stride(0) * bufs[n].element_size())
                io.counts = counts.data_ptr()
                ios.append(io)
            med, spread = timed(lambda b: ctx.call("mdvt_export_geometry_batch", F, params[b], C.byref(opts), C.byref(ios[b]), stream))
            # the algorithmic traffic of the batches the windows cycled through, from the counts of each
            traffic = 0
            for b in range(B):
                ctx.call("mdvt_export_geometry_batch", F, params[b], C.byref(opts), C.byref(ios[b]), stream)
                cnt = counts.cpu().numpy().astype(np.int64)
                for U, M in cnt:
                    n_of = {"vertices": N, "triangles": int(M), "used_index": int(U), "points": int(U), "point_rgb": int(U)}
                    traffic += 3 * N + (3 * N if "point_rgb" in want else 0) + 8 + sum(ITEM[n] * n_of[n] for n in want)
            per_call = traffic / B
            line = dict(what="export_geometry", size=f"{W}x{H}", frames=F, remove_edges=remove, outputs=name, ms_per_frame=med * 1e3 / F,
                        spread=spread, frames_per_s=F / med, algorithmic_bytes_per_frame=per_call / F, achieved_GB_per_s=per_call / med / 1e9,
                        used_fraction=float(cnt[:, 0].mean() / N), kept_fraction=float(cnt[:, 1].mean() / (2 * ncell)))
            print(json.dumps(line), flush=True)
            lines.append(line)
    for bits in (16, 8):
        row = (2 if bits == 16 else 3) * W
        out = torch.empty((F, H, row), dtype=torch.uint8, device="cuda")
        med, spread = timed(lambda b: ctx.call("mdvt_depth_grey_batch", F, depth[b].data_ptr(), 3 * W, 3 * N, 100.0, bits, out.data_ptr(), row, row * H, stream))
        line = dict(what="depth_grey", size=f"{W}x{H}", frames=F, bits=bits, ms_per_frame=med * 1e3 / F, spread=spread, frames_per_s=F / med,
                    algorithmic_bytes_per_frame=3 * N + row * H, achieved_GB_per_s=F * (3 * N + row * H) / med / 1e9)
        print(json.dumps(line), flush=True)
        lines.append(line)
    ctx.close()
    # the restatement on this box's CPU, one frame (NumPy and the C oracle, single-threaded)
    d0, c0 = fr[0][0], fr[0][1]
    for remove in (1, 0):
        t0 = time.perf_counter()
        ref = gr.export(d0, K, decode=0, remove_edges=remove, T=np.asarray(track[0]).reshape(4, 4), color_rgb=c0)
        line = dict(what="geometry_ref on the host", size=f"{W}x{H}", remove_edges=remove, s_per_frame=time.perf_counter() - t0, counts=list(ref.counts))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
