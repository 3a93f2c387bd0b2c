"""Times of the host-side share of the StereoCrafter infill step on one chunk: the four entry points of
include/mdvt_infill_adapter.h on 25 side-by-side frames of 3840 x 1080 (the reference's chunk, scr:222) around a model of
1024 x 768, per call and in total, and the NumPy / SciPy restatement of the same work (tests/infill_adapter_ref.py, with
mark_lower_side from the C oracle) on this box.

    python tools/infill_adapter_bench.py [--frames 25] [--size 3840x1080] [--model 1024x768] [--reps 7] [--numpy-frames 3]
                                         [--skip-numpy] [--md profiles/r11_infill_adapter.md] [--json out.json]

The model itself is not run: its place is taken by the prepared frames (any uint8 frames of the model's size cost the same).  Each
device call is timed with events around it after a warm-up call; medians of --reps warmed runs are reported with the fastest.  The
NumPy side runs --numpy-frames frames of the chunk once and is scaled to the chunk (it is a per-frame loop); the reference's own
mark_lower_side is a Python loop over the marching pixels per step and slower still than the C oracle's that stands in for it here.
The first frames of every device result are compared with the restatement before anything is timed.

Like tools/metric_convert_bench.py this tool takes NumPy's side -- and with it the lower-side marks' plain-C stand-in -- from the test
tree: it runs from a source checkout."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    return float(np.median(ms)), min(ms)


def chunk(n, W2, H, seed=3):
    """Colour frames with structure and infill masks with a few per cent of holes along vertical object edges (normal-coloured)."""
    rng = np.random.default_rng(seed)
    ew = W2 // 2
    y, x = np.mgrid[0:H, 0:W2]
    color = np.empty((n, H, W2, 3), dtype=np.uint8)
    mask = np.zeros((n, H, W2, 3), dtype=np.uint8)
    for t in range(n):
        color[t] = np.stack([(x + 3 * t) % 256, (y + x // 4) % 256, (x // 3 + y // 2 + 5 * t) % 256], axis=-1)
        for eye in (0, 1):
            for k in range(6):
                x0 = eye * ew + int(rng.integers(20, ew - 60))
                y0, h, w = int(rng.integers(0, H // 2)), int(rng.integers(H // 4, H // 2)), int(rng.integers(8, 40))
                mask[t, y0:y0 + h, x0:x0 + w] = (255, 127, 1) if eye else (0, 128, 255)
    return color, mask


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--size", default="3840x1080")
    ap.add_argument("--model", default="1024x768")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-frames", type=int, default=3)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import torch
    import infill_adapter_ref as R
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    marks = R.lower_side_oracle()                                             # (the tools never import the checker themselves)
    n = a.frames
    W2, H = (int(v) for v in a.size.split("x"))
    model = tuple(int(v) for v in a.model.split("x"))
    color, mask = chunk(n, W2, H)
    holes = float((mask != 0).any(axis=-1).mean())
    d_color, d_mask = torch.from_numpy(color).cuda(), torch.from_numpy(mask).cuda()
    pasted, blended = torch.empty_like(d_color), torch.empty_like(d_color)

    # ---- correctness first: two frames of every call against the restatement
    k = min(n, 2)
    for eye in (0, 1):
        image, mmask, counts = sci.prepare_eye(d_color[:k], d_mask[:k], eye, model)
        wi, wm, wc = R.prepare_eye(color[:k], mask[:k], eye, *model)
        assert np.array_equal(image.cpu().numpy(), wi) and np.array_equal(mmask.cpu().numpy(), wm) and np.array_equal(counts.cpu().numpy(), wc.astype(np.int32))
        fake = torch.flip(image, dims=(0,)).contiguous()                       # stands in for the model's output
        got = sci.transfer_lhm_video_refmask(fake, image, mmask).cpu().numpy()
        want = R.transfer_lhm(wi[::-1], wi, wm)
        assert np.array_equal(got, want)
        sci.composite_eye(torch.from_numpy(want).cuda(), d_color[:k], d_mask[:k], eye, pasted[:k], blended[:k])
        wp, wb = R.composite_eye(want, color[:k], mask[:k], eye, marks)
        assert np.array_equal(R.eye_of(pasted[:k].cpu().numpy(), eye), wp) and np.array_equal(R.eye_of(blended[:k].cpu().numpy(), eye), wb)
    print("device results equal the restatement on the first frames", flush=True)

    # ---- the device, both eyes per row
    rows = []
    prepared = [sci.prepare_eye(d_color, d_mask, eye, model) for eye in (0, 1)]
    mom = torch.empty((3, n, 10), dtype=torch.int64, device="cuda")
    params = torch.from_numpy(sci.lhm_params(*sci.lhm_moments(prepared[0][0]).cpu().numpy()[None].repeat(3, 0))).cuda()
    matched = torch.empty_like(prepared[0][0])

    def prepare():
        for eye in (0, 1):
            sci.prepare_eye(d_color, d_mask, eye, model)

    def moments():
        for image, mmask, _ in prepared:
            sci.lhm_moments(image, None, out=mom[0])
            sci.lhm_moments(image, None, out=mom[2])
            sci.lhm_moments(image, mmask, out=mom[1])

    def apply():
        for image, _, _ in prepared:
            sci.lhm_apply(image, params, out=matched)

    def composite():
        for eye, (image, _, _) in enumerate(prepared):
            sci.composite_eye(image, d_color, d_mask, eye, pasted, blended)

    def match():                                                              # as the module runs it: with its read-back and host algebra
        for image, mmask, _ in prepared:
            sci.transfer_lhm_video_refmask(image, image, mmask)

    def total():
        prepare()
        match()
        composite()

    for name, fn in (("mdvt_adapter_prepare_eye", prepare), ("mdvt_lhm_moments (3 per eye)", moments), ("mdvt_lhm_apply", apply),
                     ("mdvt_adapter_composite_eye", composite), ("colour match incl. read-back + host algebra", match),
                     ("all four, both eyes, one chunk", total)):
        med, best = timed(torch, fn, a.reps)
        rows.append(dict(what=name, ms_median=med, ms_best=best))
        print(f"{name:<46} median {med:9.3f} ms   best {best:9.3f} ms", flush=True)

    # ---- NumPy / SciPy on this box
    host = []
    if not a.skip_numpy:
        kk = min(n, a.numpy_frames)
        t_prep = t_match = t_comp = 0.0
        for eye in (0, 1):
            t0 = time.perf_counter()
            wi, wm, _ = R.prepare_eye(color[:kk], mask[:kk], eye, *model)
            t1 = time.perf_counter()
            wt = R.transfer_lhm(wi, wi, wm)
            t2 = time.perf_counter()
            R.composite_eye(wt, color[:kk], mask[:kk], eye, marks)
            t3 = time.perf_counter()
            t_prep, t_match, t_comp = t_prep + (t1 - t0), t_match + (t2 - t1), t_comp + (t3 - t2)
        scale = n / kk
        for name, t in (("prepare (resize, both eyes)", t_prep), ("colour match", t_match), ("composite (C mark_lower_side, SciPy dilation, Gaussian, blend)", t_comp),
                        ("all, both eyes, one chunk", t_prep + t_match + t_comp)):
            host.append(dict(what=name, ms_measured=t * 1e3, frames=kk, ms_scaled_to_chunk=t * 1e3 * scale))
            print(f"NumPy {name:<60} {t * 1e3:10.1f} ms for {kk} frame(s) -> {t * 1e3 * scale:10.1f} ms per chunk of {n}", flush=True)

    box = f"{torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; torch {torch.__version__}"
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(box=box, frames=n, size=a.size, model=a.model, hole_share=holes, device=rows, numpy=host), f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# The infill adapter on one chunk\n\n")
            f.write(f"`python tools/infill_adapter_bench.py --frames {n} --size {a.size} --model {a.model} --reps {a.reps} --numpy-frames {a.numpy_frames}`\n\n")
            f.write(f"Box: {box}.\n\n")
            f.write(f"{n} side-by-side frames of {a.size}, model {a.model}, {100 * holes:.1f} % of the pixels under the infill mask.  The model is not run.  "
                    f"Device times: events around the calls of both eyes, median (and fastest) of {a.reps} warmed runs.\n\n")
            f.write("| device, both eyes | median ms | fastest ms |\n|---|---:|---:|\n")
            for r in rows:
                f.write(f"| {r['what']} | {r['ms_median']:.3f} | {r['ms_best']:.3f} |\n")
            if host:
                f.write(f"\nNumPy / SciPy restatement (tests/infill_adapter_ref.py; mark_lower_side from the C oracle) on the same box, one run of "
                        f"{host[0]['frames']} frame(s), scaled to the chunk (the work is a per-frame loop).  The reference's own mark_lower_side is a "
                        "Python loop per marching step and slower still; it was not measured.\n\n")
                f.write("| host, both eyes | measured ms | scaled to the chunk, ms |\n|---|---:|---:|\n")
                for r in host:
                    f.write(f"| {r['what']} | {r['ms_measured']:.1f} | {r['ms_scaled_to_chunk']:.1f} |\n")
            f.write("\nNot measured: the model, the file decode and encode around the chunk, and the reference's own script (it needs OpenCV and the model).\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
