"""Times of the host-side share of the m2svid and stereo_dissoclusion_net infill steps (include/mdvt_infill_engines.h), everything but
the models, on the same box:

  1. one m2svid chunk: 25 side-by-side frames of 3840 x 1080 and their 1920 x 1080 originals, both eyes -- mdvt_m2svid_prepare_eye to
     512 x 512 / 64 x 64 and mdvt_adapter_composite_eye back from 512 x 512;
  2. mdvt_model_infill_finish on 16 side-by-side frames of 3840 x 1080 (one call per eye, as the module makes them);
  3. mdvt_normal_infill on the same frames and masks, alternating with 2 in the same loop: the finish does a subset of its work;
  4. the NumPy / SciPy / plain-C restatement of 1 and 2 (tests/infill_engines_ref.py) on a few frames, scaled.

    python tools/infill_engines_bench.py [--chunk 25] [--finish-frames 16] [--size 3840x1080] [--reps 9] [--numpy-frames 2]
                                         [--skip-numpy] [--md profiles/r13_infill_engines.md] [--json out.json]

The models are not run: for m2svid the prepared frames take the place of the model's, for the finish a shifted copy of the rendered
frame does (any uint8 image of the right size costs the same).  Device calls are timed with events around them after a warm-up call;
medians of --reps warmed runs are reported with the fastest.  The first frames of every device result are compared with the
restatement before anything is timed.

Like tools/infill_adapter_bench.py this tool takes the host's side -- and with it the plain-C stand-ins for the reference's Python
loops -- from the test tree: it runs from a source checkout."""
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


def timed(torch, fns, reps):
    """Medians and fastest times (ms) of the functions of `fns`, run in turn within each repetition (alternating: what disturbs one
    disturbs the other)."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(float(np.median(m)), min(m)) for m in ms]


def frames(n, W2, H, seed=3):
    """Colour frames with structure and infill masks with a few per cent of holes along vertical object edges, normal-coloured with
    no zero channel (every hole pixel is bg for the finish), and their original frames of one eye's size."""
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
                mask[t, y0:y0 + h, x0:x0 + w] = (255, 127, 1) if eye else (1, 128, 255)
    org = np.ascontiguousarray(color[:, :, ew // 2: ew // 2 + ew])
    return color, mask, org


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=25)
    ap.add_argument("--finish-frames", type=int, default=16)
    ap.add_argument("--size", default="3840x1080")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--numpy-frames", type=int, default=2)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--md", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    import torch
    import infill_adapter_ref as R
    import infill_engines_ref as E
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    host_c = R.lower_side_oracle()                                            # (the tools never import the checker themselves)
    W2, H = (int(v) for v in a.size.split("x"))
    ew = W2 // 2
    n, nf = a.chunk, a.finish_frames
    image_size, mask_size = (m2s.IMAGE_W, m2s.IMAGE_H), (m2s.MASK_W, m2s.MASK_H)
    color, mask, org = frames(max(n, nf), W2, H)
    holes = float((mask != 0).any(axis=-1).mean())
    d_color, d_mask, d_org = torch.from_numpy(color).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(org).cuda()
    d_model = torch.roll(d_color, shifts=5, dims=2).contiguous()              # stands in for the net's image
    pasted, blended = torch.empty_like(d_color[:n]), torch.empty_like(d_color[:n])
    out_f, out_n = torch.empty_like(d_color[:nf]), torch.empty_like(d_color[:nf])
    halves = (slice(0, ew), slice(ew, 2 * ew))

    # ---- correctness first: the first frame of every call against the restatement
    for eye in (0, 1):
        got = m2s.prepare_eye(d_color[:1], d_mask[:1], d_org[:1], eye, image_size, mask_size)
        want = E.m2s_prepare_eye(color[:1], mask[:1], org[:1], eye, image_size, mask_size)
        assert all(np.array_equal(g.cpu().numpy(), w.astype(np.int32) if w.dtype == np.uint32 else w) for g, w in zip(got, want))
        sci.composite_eye(got[0], d_color[:1], d_mask[:1], eye, pasted[:1], blended[:1])
        wp, wb = R.composite_eye(want[0], color[:1], mask[:1], eye, host_c)
        assert np.array_equal(R.eye_of(pasted[:1].cpu().numpy(), eye), wp) and np.array_equal(R.eye_of(blended[:1].cpu().numpy(), eye), wb)
        h = halves[eye]
        sdn.model_infill_finish(d_color[:1, :, h], d_model[:1, :, h], d_mask[:1, :, h], out=out_f[:1, :, h])
        want = E.finish(np.ascontiguousarray(color[0, :, h]), d_model[0, :, h].cpu().numpy(), np.ascontiguousarray(mask[0, :, h]), host_c)
        assert np.array_equal(out_f[0, :, h].cpu().numpy(), want)
    print("device results equal the restatement on the first frame", flush=True)

    # ---- the device, both eyes per row
    prepared = [m2s.prepare_eye(d_color[:n], d_mask[:n], d_org[:n], eye, image_size, mask_size) for eye in (0, 1)]

    def prepare():
        for eye in (0, 1):
            m2s.prepare_eye(d_color[:n], d_mask[:n], d_org[:n], eye, image_size, mask_size)

    def composite():
        for eye in (0, 1):
            sci.composite_eye(prepared[eye][0], d_color[:n], d_mask[:n], eye, pasted, blended)

    def chunk():
        prepare()
        composite()

    def finish():
        for h in halves:
            sdn.model_infill_finish(d_color[:nf, :, h], d_model[:nf, :, h], d_mask[:nf, :, h], out=out_f[:, :, h])

    def normal_infill():
        bni.normal_infill_sbs(d_color[:nf], d_mask[:nf], out=out_n)

    rows = []
    names = [f"mdvt_m2svid_prepare_eye, {n} frames", f"mdvt_adapter_composite_eye from 512 x 512, {n} frames", f"one m2svid chunk: both, {n} frames"]
    for name, (med, best) in zip(names, timed(torch, (prepare, composite, chunk), a.reps)):
        rows.append(dict(what=name, ms_median=med, ms_best=best))
    names = [f"mdvt_model_infill_finish, {nf} frames", f"mdvt_normal_infill, the same {nf} frames"]
    for name, (med, best) in zip(names, timed(torch, (finish, normal_infill), a.reps)):
        rows.append(dict(what=name, ms_median=med, ms_best=best))
    for r in rows:
        print(f"{r['what']:<58} median {r['ms_median']:9.3f} ms   best {r['ms_best']:9.3f} ms", flush=True)

    # ---- NumPy / SciPy / plain C on this box
    host = []
    if not a.skip_numpy:
        kk = max(1, min(n, nf, a.numpy_frames))
        t_prep = t_comp = t_fin = 0.0
        for eye in (0, 1):
            t0 = time.perf_counter()
            wi = E.m2s_prepare_eye(color[:kk], mask[:kk], org[:kk], eye, image_size, mask_size)[0]
            t1 = time.perf_counter()
            R.composite_eye(wi, color[:kk], mask[:kk], eye, host_c)
            t2 = time.perf_counter()
            h = halves[eye]
            model = np.roll(color[:kk], 5, axis=2)[:, :, h]
            E.finish(np.ascontiguousarray(color[:kk, :, h]), np.ascontiguousarray(model), np.ascontiguousarray(mask[:kk, :, h]), host_c)
            t3 = time.perf_counter()
            t_prep, t_comp, t_fin = t_prep + (t1 - t0), t_comp + (t2 - t1), t_fin + (t3 - t2)
        for name, t, frames_to in ((f"m2svid prepare (three resizes per eye)", t_prep, n), ("m2svid composite (C mark_lower_side, SciPy dilation, Gaussian, blend)", t_comp, n),
                                   ("one m2svid chunk: both", t_prep + t_comp, n), ("the finish (plain-C box mean, march, dilation, masked Gaussian)", t_fin, nf)):
            host.append(dict(what=name, ms_measured=t * 1e3, frames=kk, scaled_to_frames=frames_to, ms_scaled=t * 1e3 * frames_to / kk))
            print(f"host  {name:<70} {t * 1e3:10.1f} ms for {kk} frame(s) -> {t * 1e3 * frames_to / kk:10.1f} ms for {frames_to}", flush=True)

    box = f"{torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; torch {torch.__version__}"
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(box=box, chunk=n, finish_frames=nf, size=a.size, hole_share=holes, device=rows, host=host), f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# The m2svid and stereo_dissoclusion_net infill steps around their models\n\n")
            f.write(f"`python tools/infill_engines_bench.py --chunk {n} --finish-frames {nf} --size {a.size} --reps {a.reps} --numpy-frames {a.numpy_frames}`\n\n")
            f.write(f"Box: {box}.\n\n")
            f.write(f"Side-by-side frames of {a.size} with originals of {ew} x {H}, {100 * holes:.1f} % of the pixels under the infill mask, model inputs "
                    f"{image_size[0]} x {image_size[1]} and {mask_size[0]} x {mask_size[1]}.  The models are not run.  Device times: events around the calls "
                    f"of both eyes, median (and fastest) of {a.reps} warmed runs; the calls of a group alternate within each repetition.\n\n")
            f.write("| device, both eyes | median ms | fastest ms |\n|---|---:|---:|\n")
            for r in rows:
                f.write(f"| {r['what']} | {r['ms_median']:.3f} | {r['ms_best']:.3f} |\n")
            fin, ni = rows[3]["ms_median"], rows[4]["ms_median"]
            f.write(f"\nThe finish against mdvt_normal_infill on the same frames and masks: {fin:.3f} ms against {ni:.3f} ms ({fin / ni:.2f} x).\n")
            if host:
                f.write(f"\nNumPy / SciPy restatement with the plain-C stand-ins for the reference's Python loops (tests/infill_engines_ref.py) on the same "
                        f"box, one run of {host[0]['frames']} frame(s), scaled (the work is a per-frame loop).  The reference's own loops are slower "
                        "still; they were not measured.\n\n")
                f.write("| host, both eyes | measured ms | scaled, ms | scaled to frames |\n|---|---:|---:|---:|\n")
                for r in host:
                    f.write(f"| {r['what']} | {r['ms_measured']:.1f} | {r['ms_scaled']:.1f} | {r['scaled_to_frames']} |\n")
            f.write("\nNot measured: the models, the file decode and encode around the calls, and the reference's own scripts (they need OpenCV and the "
                    "models).  Not observed: cv2's resize, blur and Gaussian (restated), and both default model wrappers.\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
