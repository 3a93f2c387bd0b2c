#!/usr/bin/env python3
"""Times the three entry points of include/mdvt_video_mask.h on the GPU, at 16 x 1920x1080 and 8 x 3840x2160, next to a device copy
of the same bytes and next to the route the reference takes -- the frames to the host, Pillow per frame, back to the device:

    python tools/video_mask_bench.py [--calls 20] [--clips] [--json out.json] [--md out.md]

Per size, in one series whose calls alternate:
  model_input      mdvt_mask_model_input: the frames to the float32 tensor [n, 3, 320, 320]
  mask             mdvt_mask_from_prediction: float32 [n, 320, 320] to the mask video's frames [n, H, W, 3]
  resize fused     mdvt_lanczos_resize_u8, RGB frames to 320 x 320, the fused LDS form
  resize two       the same in the two-launch form (the comparison that decides the library's choice)
  resize mask      mdvt_lanczos_resize_u8, mode L, 320 x 320 to the frames' size (an enlarging resize: two launches)
  copy             torch's copy_ of the frames' bytes on the device: what moving the input once costs
  host route       D2H of the frames, Image.resize(LANCZOS) and rembg's normalize per frame on a pool of the usable cores (at most
                   16), H2D of the tensor; then D2H of the bytes, Image.resize per mask, H2D.  Skipped where Pillow is missing.
Medians of --calls calls with quartiles, device events (the host route: a host clock around work that ends in a synchronise).

--clips: tools/generate_video_mask.py on a 300-frame 960x540 clip with a stub model on the device, per codec pair.  Nothing here
runs without a GPU."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
S = 320
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _tool():
    spec = importlib.util.spec_from_file_location("generate_video_mask_tool", os.path.join(REPO, "tools", "generate_video_mask.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _stats(v):
    return dict(median_ms=float(np.median(v)), quartiles_ms=[float(np.percentile(v, 25)), float(np.percentile(v, 75))])


def _cores():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


def bench_size(torch, _lib, ctx, n, W, H, calls):
    L = _lib.load()
    stream = _lib.stream_arg(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(19)
    frames = torch.randint(0, 256, (n, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    frames_copy = torch.empty_like(frames)
    x = torch.empty((n, 3, S, S), dtype=torch.float32, device="cuda")
    pred = torch.rand((n, S, S), generator=g, device="cuda")
    mask = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    small = torch.empty((n, S, S, 3), dtype=torch.uint8, device="cuda")
    grey = torch.randint(0, 256, (n, S, S), generator=g, device="cuda", dtype=torch.uint8)
    big = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    d3 = C.c_double * 3
    h_mean, h_std = d3(*MEAN), d3(*STD)
    mean, std = C.cast(h_mean, C.c_void_p), C.cast(h_std, C.c_void_p)

    def resize(src, dst, ch, w, h, ow, oh, form):
        return lambda: ctx.check(L.mdvt_lanczos_resize_u8(ctx.handle, w, h, ch, n, src.data_ptr(), ch * w, ch * w * h, ow, oh, dst.data_ptr(), ch * ow,
                                                          ch * ow * oh, form, None, stream))
    series = {
        "model_input": lambda: ctx.check(L.mdvt_mask_model_input(ctx.handle, W, H, n, frames.data_ptr(), 3 * W, 3 * W * H, 0, S, S, mean, std,
                                                                 x.data_ptr(), 4 * S, 4 * S * S, 12 * S * S, stream)),
        "mask": lambda: ctx.check(L.mdvt_mask_from_prediction(ctx.handle, S, S, n, pred.data_ptr(), 4 * S, 4 * S * S, W, H, 3, mask.data_ptr(), 3 * W,
                                                              3 * W * H, stream)),
        "resize fused": resize(frames, small, 3, W, H, S, S, _lib.LANCZOS_FUSED),
        "resize two": resize(frames, small, 3, W, H, S, S, _lib.LANCZOS_TWO_LAUNCH),
        "resize mask": resize(grey, big, 1, S, S, W, H, _lib.LANCZOS_AUTO),
        "copy": lambda: frames_copy.copy_(frames),
    }
    # the two forms give the same bytes at this size
    series["resize fused"]()
    fused = small.clone()
    series["resize two"]()
    same = bool(torch.equal(fused, small))
    for _ in range(2):                                              # every shape is warmed before it is timed
        for fn in series.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in series}
    for _ in range(calls):
        for k, fn in series.items():
            t[k].append(_timed(torch, fn))
    row = dict(frames=n, size=[W, H], calls=calls, forms_equal=same, input_bytes=n * W * H * 3, mask_bytes=n * W * H * 3,
               times={k: _stats(v) for k, v in t.items()})
    try:
        from PIL import Image
    except ImportError:
        row["host_route"] = "not measured: Pillow is not importable on this machine"
        return row
    from concurrent.futures import ThreadPoolExecutor
    cores = _cores()

    def one_in(f):
        im = np.array(Image.fromarray(f, "RGB").resize((S, S), Image.LANCZOS))
        im = im / max(np.max(im), 1e-6)
        return np.stack([(im[:, :, c] - MEAN[c]) / STD[c] for c in range(3)]).astype(np.float32)

    def one_out(p):
        ma, mi = np.max(p), np.min(p)
        m = np.asarray(Image.fromarray(((p - mi) / (ma - mi) * 255).astype("uint8"), "L").resize((W, H), Image.LANCZOS))
        return np.repeat(m[..., None], 3, axis=-1)
    with ThreadPoolExecutor(cores) as pool:
        def host_in():
            x.copy_(torch.from_numpy(np.stack(list(pool.map(one_in, frames.cpu().numpy())))))

        def host_out():
            mask.copy_(torch.from_numpy(np.stack(list(pool.map(one_out, pred.cpu().numpy())))))
        reps = max(3, calls // 4)
        host_in(), host_out()
        row["host_route"] = dict(cores=cores, calls=reps, model_input=_stats([_wall(torch, host_in) for _ in range(reps)]),
                                 mask=_stats([_wall(torch, host_out) for _ in range(reps)]))
    return row


def stub_model(x):
    """A stand-in for the network, on the device: a fixed mix of the three planes at half the size."""
    x = x[:, :, ::2, ::2]
    return (x[:, 0] * 0.5 + x[:, 1] * 0.25 - x[:, 2] * 0.125).contiguous()


def bench_clips():
    import torch
    from metric_depth_video_toolbox_amd import video_io, video_mask
    tool = _tool()
    W, H, n = 960, 540, 300
    rows = []
    with tempfile.TemporaryDirectory() as d:
        base = np.random.default_rng(n).integers(0, 256, (H, W, 3), dtype=np.uint8)
        clip = os.path.join(d, f"clip{n}.mkv")
        with video_io.VideoWriter(clip, W, H, 24.0) as wr:
            for k in range(n):
                wr.write(np.roll(base, 3 * k, axis=1))
        parse = video_mask.build_parser().parse_args
        tool.run(parse(["--color_video", clip, "--batch_size", "16", "--max_frames", "32"]), stub_model)      # the first run warms the process
        for dec, enc in (("host", "host"), ("device", "host"), ("host", "device"), ("device", "device")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tool.run(parse(["--color_video", clip, "--batch_size", "16", "--video_decoder", dec, "--video_encoder", enc]), stub_model)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            rows.append(dict(frames=n, size=[W, H], decoder=dec, encoder=enc, seconds=s, frames_per_s=n / s))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def markdown(out):
    lines = ["# r19: the mask-video step's entry points", "",
             "Written by `tools/video_mask_bench.py --clips --md` on an MI355X.  Milliseconds are medians (quartiles in brackets) of the calls "
             "named per row, timed by device events in one series whose calls alternate; the host route is timed by a host clock around work "
             "that ends in a device synchronise.  There is no pass mark on speed.", ""]
    names = ["model_input", "mask", "resize fused", "resize two", "resize mask", "copy"]
    lines += ["| frames | " + " | ".join(names) + " | host route: model input | host route: mask |", "|---|" + "---|" * (len(names) + 2)]
    for r in out["calls"]:
        cell = lambda s: f"{s['median_ms']:.3f} [{s['quartiles_ms'][0]:.3f}, {s['quartiles_ms'][1]:.3f}]"
        hr = r["host_route"]
        host = [cell(hr["model_input"]), cell(hr["mask"])] if isinstance(hr, dict) else [hr, hr]
        lines.append(f"| {r['frames']} x {r['size'][0]}x{r['size'][1]} ({r['calls']} calls) | " + " | ".join(cell(r["times"][k]) for k in names) +
                     " | " + " | ".join(host) + " |")
    lines.append("")
    for r in out["calls"]:
        f, t = r["times"]["resize fused"]["median_ms"], r["times"]["resize two"]["median_ms"]
        lines.append(f"- {r['frames']} x {r['size'][0]}x{r['size'][1]} to 320x320: the fused LDS form takes {f:.3f} ms, the two-launch form {t:.3f} ms "
                     f"(fused / two launches = {f / t:.2f}); the two forms' bytes are equal: {r['forms_equal']}.")
        if isinstance(r["host_route"], dict):
            lines.append(f"  The host route ran Pillow on {r['host_route']['cores']} threads, {r['host_route']['calls']} calls.")
    if out.get("clips"):
        lines += ["", "`tools/generate_video_mask.py` on a 300-frame 960x540 clip with a stub model on the device, batches of 16, wall clock around "
                  "the whole step (decode, the two entry points, the stub, encode, the file):", "", "| decoder | encoder | seconds | frames/s |",
                  "|---|---|---|---|"]
        for r in out["clips"]:
            lines.append(f"| {r['decoder']} | {r['encoder']} | {r['seconds']:.2f} | {r['frames_per_s']:.0f} |")
    return "\n".join(lines) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=20, help="timed calls per case")
    p.add_argument("--clips", action="store_true", help="also time the whole tool on a 300-frame clip with a stub model")
    p.add_argument("--json", default=None, help="write all rows to this file")
    p.add_argument("--md", default=None, help="write the rows as a markdown report to this file")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("video_mask_bench needs a GPU: a timing taken elsewhere says nothing about it")
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    out = dict(calls=[])
    try:
        for n, W, H in ((16, 1920, 1080), (8, 3840, 2160)):
            out["calls"].append(bench_size(torch, _lib, ctx, n, W, H, args.calls))
            print(json.dumps(out["calls"][-1]), flush=True)
    finally:
        ctx.close()
    if args.clips:
        out["clips"] = bench_clips()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(markdown(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
