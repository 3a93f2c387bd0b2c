"""Rates of the relative-to-metric conversion (video_metric_convert): the scale-and-shift fit and the codes call, on device tensors,
and the same lines run by NumPy on this box for orientation.

    python tools/metric_convert_bench.py [--fit 32x518x924] [--frames 128] [--size 924x518] [--out 1920x1080] [--reps 7]
                                         [--calls-only N] [--skip-numpy] [--json out.json]

The fit: --fit frames x height x width, with and without a uint8 mask, the target given as depth (the library's own inverse); bytes/s
counts the algorithmic 8 B per element (+ 1 B of mask).  The codes: --frames planes of --size, same size and resized to --out, both
styles, with and without the depth planes; bytes/s counts 4 B per source pixel read and 3 B (+ 4 B of depth plane) per output pixel
written.  Each call is timed with events around it after a warm-up call; the fastest of --reps is reported with the median.  The first
result of every kind is compared with NumPy's (tests/metric_align_ref.py) on a few frames before anything is timed.  --calls-only N
just makes N calls of each kind (for a kernel trace).

Like tools/find_convergence_bench.py this tool takes NumPy's side from the test tree (tests/metric_align_ref.py, put on sys.path
below): it runs from a source checkout, not from an installation without tests/."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), float(np.median(ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit", default="32x518x924")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--size", default="924x518")
    ap.add_argument("--out", default="1920x1080")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls-only", type=int, default=0)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import torch
    import metric_align_ref as mr
    from metric_depth_video_toolbox_amd import video_metric_convert as vmc
    rows = []

    def report(what, case, ms, med, nbytes, units, unit):
        r = dict(what=what, case=case, ms=ms, ms_median=med, gbytes_per_s=nbytes / (ms * 1e-3) / 1e9, per_s=units / (ms * 1e-3), unit=unit)
        rows.append(r)
        print(f"{what:>12} {case:<46} {ms:8.3f} ms (median {med:8.3f})  {r['gbytes_per_s']:8.1f} GB/s  {r['per_s']:12.0f} {unit}/s", flush=True)

    # ---- the fit
    N, H, W = (int(v) for v in a.fit.split("x"))
    rng = np.random.default_rng(1)
    p, d = mr.gen_model(rng, N, H, W)
    m = mr.gen_mask(rng, N, H, W, values=(0, 1))
    dp, dd, dm = torch.from_numpy(p).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(m).cuda()
    t = mr.inverse(d)
    for case, mask, dmask in (("no mask", None, None), ("uint8 mask", m, dm)):
        want = mr.fit(mr.concat(p), mr.concat(t), None if mask is None else mr.concat(mask))
        got = vmc.compute_scale_and_shift_full(dp, dd, dmask, target_is_depth=True).numpy()
        assert mr.same_bits(got, want).size == 0, (case, got, want)
        call = lambda: vmc.compute_scale_and_shift_full(dp, dd, dmask, target_is_depth=True)
        if a.calls_only:
            for _ in range(a.calls_only):
                call()
            torch.cuda.synchronize()
            continue
        ms, med = timed(torch, call, a.reps)
        report("fit", f"{a.fit} {case}", ms, med, N * H * W * (8 if mask is None else 9), N * H * W, "elements")
        if not a.skip_numpy:
            t0 = time.perf_counter()
            mr.fit(mr.concat(p), mr.inverse(mr.concat(d)), None if mask is None else mr.concat(mask))
            dt = time.perf_counter() - t0
            report("NumPy fit", f"{a.fit} {case}", dt * 1e3, dt * 1e3, N * H * W * (8 if mask is None else 9), N * H * W, "elements")

    # ---- the codes
    n = a.frames
    w, h = (int(v) for v in a.size.split("x"))
    ow, oh = (int(v) for v in a.out.split("x"))
    x = (rng.random((n, h, w), dtype=np.float32) * np.float32(3)).astype(np.float32)
    dx = torch.from_numpy(x).cuda()
    fit = torch.tensor([0.3712, 0.0113], dtype=torch.float32, device="cuda")
    for style in (0, 1):
        for out_size in (None, (ow, oh)):
            k = min(n, 2)
            want_codes, want_depth = mr.metric_codes(x[:k], 0.3712, 0.0113, 100, style, out_size)
            codes, depth = vmc.metric_depth_codes(dx[:k], fit, 100, style=style, out_size=out_size, want_depth=True)
            assert np.array_equal(codes.cpu().numpy(), want_codes) and mr.same_bits(depth.cpu().numpy(), want_depth).size == 0, (style, out_size)
            tw, th = (w, h) if out_size is None else out_size
            out = torch.empty((n, th, tw, 3), dtype=torch.uint8, device="cuda")
            for want_d in (False, True):
                call = lambda: vmc.metric_depth_codes(dx, fit, 100, style=style, out_size=out_size, want_depth=want_d, out=out)
                if a.calls_only:
                    for _ in range(a.calls_only):
                        call()
                    torch.cuda.synchronize()
                    continue
                ms, med = timed(torch, call, a.reps)
                case = f"{n} x {w}x{h}" + ("" if out_size is None else f" -> {tw}x{th}") + f" style {style}" + (" + depth planes" if want_d else "")
                report("codes", case, ms, med, n * (4 * w * h + (7 if want_d else 3) * tw * th), n * tw * th, "output px")
            if not a.skip_numpy and not a.calls_only:
                kk = min(n, 8)
                t0 = time.perf_counter()
                mr.metric_codes(x[:kk], 0.3712, 0.0113, 100, style, out_size)
                dt = time.perf_counter() - t0
                report("NumPy codes", f"{kk} x {w}x{h}" + ("" if out_size is None else f" -> {tw}x{th}") + f" style {style}", dt * 1e3, dt * 1e3,
                       kk * (4 * w * h + 7 * tw * th), kk * tw * th, "output px")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
