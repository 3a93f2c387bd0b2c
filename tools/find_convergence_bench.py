"""Rates of the convergence-depth step (find_convergence_depth): the device call alone, the file route with either decoder, and the
reference's host route (host decode + the NumPy lines of find_convergence_depth.py:53-80) on the same box.

    python tools/find_convergence_bench.py [--size 1920x1080] [--frames 128] [--reps 5] [--file-frames 64] [--skip-files]
                                           [--calls-only N] [--json out.json]

The device call: --frames frames of --size per call, already on the device, without a mask, with a mask that selects a box of about
a fifth of the frame, and with a mask that selects every pixel; timed with events around --reps calls after one warm-up call, the
fastest call reported; bytes/s counts what the call must read (3 B/px of depth, + 3 B/px of mask).  The first call's means are
compared with NumPy's before anything is timed.  --calls-only N just makes N calls of each kind (for a kernel trace)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def inputs(W, H, n, rng):
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    sc = SyntheticScene(W, H, config_id=1, n_fg=6)
    depth = np.empty((n, H, W, 3), np.uint8)
    for t in range(n):
        depth[t] = sc.frame(t % 16)[0]
    box = np.zeros((n, H, W, 3), np.uint8)
    for t in range(n):
        x0, y0 = (7 * t) % (W // 2), (3 * t) % (H // 2)
        box[t, y0:y0 + H * 2 // 5, x0:x0 + W // 2] = 255
    return depth, box


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--file-frames", type=int, default=64)
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import torch
    import convergence_ref as cr
    from metric_depth_video_toolbox_amd import clip, find_convergence_depth as fcd, video_io
    W, H = (int(v) for v in a.size.split("x"))
    n = a.frames
    rng = np.random.default_rng(1)
    depth, box = inputs(W, H, n, rng)
    d_depth = torch.from_numpy(depth).cuda()
    d_box = torch.from_numpy(box).cuda()
    d_all = torch.full_like(d_box, 255)
    rows = []
    kinds = (("no mask", None, None), ("box mask", d_box, box), ("all-white mask", d_all, None))
    for name, d_mask, h_mask in kinds:
        got = fcd.convergence_depths(d_depth, d_mask).cpu().numpy()
        k = min(n, 4)                                                # (NumPy's lines on a few frames: the tests hold the rest)
        want, _ = cr.clip_means(depth[:k], h_mask[:k] if h_mask is not None else None)
        assert cr.same_bits(got[:k], want).size == 0, (name, got[:k], want)
        if a.calls_only:
            for _ in range(a.calls_only):
                fcd.convergence_depths(d_depth, d_mask)
            torch.cuda.synchronize()
            continue
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fcd.convergence_depths(d_depth, d_mask)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        nbytes = n * W * H * (3 if d_mask is None else 6)
        r = dict(route="device call", case=name, size=a.size, frames=n, ms=min(ms), ms_median=float(np.median(ms)),
                 fps=n / (min(ms) * 1e-3), gbytes_per_s=nbytes / (min(ms) * 1e-3) / 1e9)
        rows.append(r)
        print(f"device call {name:>15} {a.size} x{n}: {r['ms']:.3f} ms (median {r['ms_median']:.3f})  {r['fps']:9.0f} frames/s  "
              f"{r['gbytes_per_s']:7.1f} GB/s of input", flush=True)
    if not a.skip_files and not a.calls_only:
        m = min(n, a.file_frames)
        tmp = tempfile.mkdtemp(prefix="fcd_bench_")
        dp, mp = os.path.join(tmp, "d.mkv"), os.path.join(tmp, "m.mkv")
        for path, frames in ((dp, depth[:m]), (mp, box[:m])):
            with video_io.VideoWriter(path, W, H, 30.0, bgr=True) as w:
                for f in frames:
                    w.write(np.ascontiguousarray(f[..., ::-1]))
        want, _ = cr.clip_means(depth[:m], box[:m])
        text = json.dumps([float(v) for v in want])

        def host_route():                                            # the reference's script with this project's host decoder
            vd, vm = clip.VideoFrames(dp), clip.VideoFrames(mp)
            out = []
            for t in range(m):
                out.append(float(cr.frame_mean(vd[t], vm[t])[0]))
            vd.close()
            vm.close()
            return json.dumps(out)
        for name, fn in (("file, host decoder", lambda: fcd.find(dp, mp, video_decoder="host") and open(dp + fcd.SIDECAR_SUFFIX).read()),
                         ("file, device decoder", lambda: fcd.find(dp, mp, video_decoder="device") and open(dp + fcd.SIDECAR_SUFFIX).read()),
                         ("host decode + NumPy", host_route)):
            assert fn() == text, name
            dt = []
            for _ in range(max(1, a.reps // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                dt.append(time.perf_counter() - t0)
            r = dict(route=name, case="box mask", size=a.size, frames=m, ms=min(dt) * 1e3, fps=m / min(dt))
            rows.append(r)
            print(f"{name:>22} box mask {a.size} x{m}: {r['ms']:.1f} ms  {r['fps']:8.1f} frames/s", flush=True)
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
