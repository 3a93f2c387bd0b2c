#!/usr/bin/env python3
"""Times the three entry points of include/mdvt_depth_engines.h on the GPU next to the obvious composition of torch operations on the
same box, in the same process:

    python tools/depth_engines_bench.py [--calls 50] [--clips] [--json out.json] [--md out.md]

The yardstick is torch, never the code under test.  The calls alternate -- torch, the entry point, torch again -- so the two torch
series, the same code on the same box, give the box's spread.  Medians of --calls calls with quartiles, timed by device events (the
torch compositions that index with a boolean mask synchronise the host inside the window: that is their cost).  Per case also the
bytes the algorithm needs over the entry point's time, against the rate of a device copy of 256 MiB of float32 (torch's copy_, 16 bytes
per lane; read plus written bytes over its time) taken in the same series, between the calls -- the yardstick tools/depth_sink_bench.py
uses as a figure from an earlier run (6.29 TB/s), here measured on the same box in the same process.

  model_frames   16 x 1920x1080 identity to float32, against permute / contiguous / float / div;
                 16 x 1920x1080 -> 1932x1092 float32, against permute / float / interpolate(bilinear) / round / div
                 (torch's bilinear is not cv2's 11-bit integer one: the same work, other bits)
  depth_prompt   16 x 1920x1080 -> 256x192, against the full-frame decode followed by interpolate(bilinear)
  focal          8 x 1920x1080 point maps [n, 3, H, W], against boolean indexing with mean, per frame and axis

--clips: the unik3d step on a 300-frame 960x540 clip through tools/depth_engine_video.py with a stub model, with host and with device
codecs.  Nothing here runs without a GPU."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_FLOATS = 64 << 20                                   # the copy yardstick: 256 MiB of float32 read, 256 MiB written


def _tool():
    spec = importlib.util.spec_from_file_location("depth_engine_video_tool", os.path.join(REPO, "tools", "depth_engine_video.py"))
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


def _series(torch, ours, yardstick, copy, calls):
    for fn in (ours, yardstick, copy, ours, yardstick, copy):   # every shape is warmed before it is timed
        fn()
    torch.cuda.synchronize()
    t = {"torch_a": [], "ours": [], "copy": [], "torch_b": []}
    for _ in range(calls):
        t["torch_a"].append(_timed(torch, yardstick))
        t["ours"].append(_timed(torch, ours))
        t["copy"].append(_timed(torch, copy))
        t["torch_b"].append(_timed(torch, yardstick))
    med = {k: float(np.median(v)) for k, v in t.items()}
    quartiles = {k: [float(np.percentile(v, 25)), float(np.percentile(v, 75))] for k, v in t.items()}
    return med, quartiles


def _row(name, med, quartiles, moved, calls, note):
    best_torch = min(med["torch_a"], med["torch_b"])
    copy_rate = 2 * 4 * COPY_FLOATS / (med["copy"] * 1e-3)         # bytes read + written per second, this series
    return dict(case=name, median_ms=med, quartiles_ms=quartiles, torch_spread_ms=abs(med["torch_a"] - med["torch_b"]),
                ours_over_torch=med["ours"] / best_torch, bytes_needed=moved, ours_bytes_per_s=moved / (med["ours"] * 1e-3),
                copy_bytes_per_s=copy_rate, share_of_copy_rate=moved / (med["ours"] * 1e-3) / copy_rate, calls=calls, note=note)


def bench_calls(args):
    import torch
    import torch.nn.functional as nnf
    from metric_depth_video_toolbox_amd import _lib
    tool = _tool()
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    rows = []
    dev = torch.device("cuda", 0)
    stream = _lib.stream_arg(dev)
    W, H = 1920, 1080
    try:
        g = torch.Generator(device="cuda").manual_seed(18)
        copy_src = torch.rand(COPY_FLOATS, generator=g, device="cuda")
        copy_dst = torch.empty_like(copy_src)
        copy = lambda: copy_dst.copy_(copy_src)
        frames = torch.randint(0, 256, (16, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
        # ---- model_frames, identity, float32 (the raw call: no Python check inside the timed window)
        out = torch.empty((16, 3, H, W), dtype=torch.float32, device="cuda")

        def ours():
            ctx.check(L.mdvt_model_frames(ctx.handle, W, H, 16, frames.data_ptr(), 3 * W, 3 * W * H, 0, W, H, 1, out.data_ptr(), 4 * W, 4 * W * H,
                                          12 * W * H, stream))
        yard = lambda: frames.permute(0, 3, 1, 2).contiguous().float().div_(255.0)
        same = bool(torch.equal(tool.model_frames(ctx, frames[:2], as_float=True), frames[:2].permute(0, 3, 1, 2).contiguous().float().div_(255.0)))
        med, q = _series(torch, ours, yard, copy, args.calls)
        rows.append(_row("model_frames 16x1920x1080 identity float32", med, q, 16 * W * H * (3 + 12), args.calls,
                         f"bit-equal to torch's GPU result: {same} (the entry point's division is NumPy's, which the tests hold it to; "
                         "torch's GPU division by a scalar need not be one division); torch runs three kernels (u8 transpose, convert, "
                         "divide in place)"))
        print(json.dumps(rows[-1]), flush=True)
        # ---- model_frames, to the next multiple of 14, float32
        w14, h14 = 1932, 1092
        out14 = torch.empty((16, 3, h14, w14), dtype=torch.float32, device="cuda")

        def ours14():
            ctx.check(L.mdvt_model_frames(ctx.handle, W, H, 16, frames.data_ptr(), 3 * W, 3 * W * H, 0, w14, h14, 1, out14.data_ptr(), 4 * w14,
                                          4 * w14 * h14, 12 * w14 * h14, stream))
        yard14 = lambda: nnf.interpolate(frames.permute(0, 3, 1, 2).float(), size=(h14, w14), mode="bilinear", align_corners=False).round_().div_(255.0)
        med, q = _series(torch, ours14, yard14, copy, args.calls)
        rows.append(_row("model_frames 16x1920x1080 -> 1932x1092 float32", med, q, 16 * (3 * W * H + 12 * w14 * h14), args.calls,
                         "torch's bilinear is float32, not cv2's 11-bit integer one: other bits"))
        print(json.dumps(rows[-1]), flush=True)
        # ---- depth_prompt
        prompt = torch.empty((16, 192, 256), dtype=torch.float32, device="cuda")
        mult = float(np.float32(100.0 / 255 ** 4))

        def ours_p():
            ctx.check(L.mdvt_depth_prompt(ctx.handle, W, H, 16, frames.data_ptr(), 3 * W, 3 * W * H, 0, 100.0, 256, 192, prompt.data_ptr(), 4 * 256,
                                          4 * 256 * 192, stream))

        def yard_p():
            d = ((frames[..., 0].long() << 24) | (frames[..., 2].long() << 16)).float() * mult
            return nnf.interpolate(d[:, None], size=(192, 256), mode="bilinear", align_corners=False)
        ours_p()
        close = float((yard_p()[:, 0] - prompt).abs().max())
        med, q = _series(torch, ours_p, yard_p, copy, args.calls)
        rows.append(_row("depth_prompt 16x1920x1080 -> 256x192", med, q, 16 * 256 * 192 * (4 * 3 + 4), args.calls,
                         f"bytes: four 3-byte taps and one float per output value; largest difference to torch's float32 bilinear {close:.3g}"))
        print(json.dumps(rows[-1]), flush=True)
        # ---- focal
        n = 8
        v, u = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
        Z = torch.rand((n, H, W), generator=g, device="cuda") * 19.5 + 0.5
        noise = 1.0 + 0.03 * torch.randn((n, 2, H, W), generator=g, device="cuda")
        X, Y = (u - W / 2) * Z / 1400.0 * noise[:, 0], (v - H / 2) * Z / 1390.0 * noise[:, 1]
        drop = torch.rand((n, H, W), generator=g, device="cuda")
        X[drop < 0.1] = 0.0
        Z[drop > 0.95] = float("nan")
        points = torch.stack([X, Y, Z], dim=1).contiguous()
        focal = torch.empty((n, 2), dtype=torch.float32, device="cuda")

        def ours_f():
            ctx.check(L.mdvt_focal_from_points(ctx.handle, W, H, n, points.data_ptr(), 0, 4 * W, 4 * W * H, 12 * W * H, focal.data_ptr(), None, stream))

        def yard_f():
            res = []
            for k in range(n):
                Xk, Yk, Zk = points[k, 0], points[k, 1], points[k, 2]
                mx, my = (Xk.abs() > 1e-6) & (Zk.abs() > 1e-6), (Yk.abs() > 1e-6) & (Zk.abs() > 1e-6)
                ex, ey = (u - W / 2.0) * (Zk / Xk), (v - H / 2.0) * (Zk / Yk)
                res.append((ex[mx].mean(), ey[my].mean()))
            return res
        ours_f()
        theirs = torch.tensor([[float(a), float(b)] for a, b in yard_f()], device="cuda")
        rel = float(((theirs - focal).abs() / theirs.abs()).max())
        med, q = _series(torch, ours_f, yard_f, copy, args.calls)
        rows.append(_row("focal_from_points 8x1920x1080 [n,3,H,W]", med, q, n * W * H * 12, args.calls,
                         f"bytes: the point maps once (the kernels read them twice and move 8 B per selected point besides); largest relative "
                         f"difference to torch's means {rel:.3g} (another order of summation)"))
        print(json.dumps(rows[-1]), flush=True)
    finally:
        ctx.close()
    return rows


def stub_unik3d(frames, cam):
    """A stand-in for the model, on the device: a quarter-size depth from the red plane, a full-size point map of a pinhole camera."""
    import torch
    n, _, H, W = frames.shape
    depth = frames[:, 0, ::4, ::4].float() / 16.0 + 0.5
    v, u = torch.meshgrid(torch.arange(H, device=frames.device, dtype=torch.float32), torch.arange(W, device=frames.device, dtype=torch.float32),
                          indexing="ij")
    Z = frames[:, 1].float() / 32.0 + 1.0
    f = 0.8 * W
    return {"depth": depth.contiguous(), "points": torch.stack([(u - W / 2) * Z / f, (v - H / 2) * Z / f, Z], dim=1)}


def bench_clips(args):
    import torch
    from metric_depth_video_toolbox_amd import depth_engines, video_io
    tool = _tool()
    W, H, n = 960, 540, 300
    rows = []
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(n)
        base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        clip = os.path.join(d, f"clip{n}.mkv")
        with video_io.VideoWriter(clip, W, H, 24.0) as wr:
            for k in range(n):
                wr.write(np.roll(base, 3 * k, axis=1))
        for k, (dec, enc) in enumerate((("host", "host"), ("device", "device"))):
            a = depth_engines.build_engine_parser().parse_args(["--engine", "unik3d", "--color_video", clip, "--batch", "16", "--video_decoder", dec,
                                                                "--video_encoder", enc])
            if k == 0:
                warm = depth_engines.build_engine_parser().parse_args(["--engine", "unik3d", "--color_video", clip, "--batch", "16", "--max_frames", "32"])
                tool.run(warm, stub_unik3d)                         # the first run warms the process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tool.run(a, stub_unik3d)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            rows.append(dict(step="unik3d", frames=n, size=[W, H], decoder=dec, encoder=enc, seconds=s, frames_per_s=n / s))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def markdown(out):
    lines = ["# r18: the depth engines' entry points next to torch", "",
             "Written by `tools/depth_engines_bench.py --clips --md` on an MI355X.  Milliseconds are medians of "
             f"{out['calls'][0]['calls']} calls (quartiles in brackets), timed by device events; the calls alternate torch, the entry point, torch, and "
             "the difference of the two torch medians is the box's spread.  Bytes are what the algorithm needs, from the shapes; the copy "
             "rate is that of a device copy of 256 MiB of float32 (torch's `copy_`; bytes read plus written over its median) timed in the same "
             "series, after each call of the entry point.  There is no pass mark on speed.", "",
             "| case | entry point ms | torch ms (first series) | torch ms (second series) | entry point / torch | GB/s | the copy's GB/s | share of the copy rate |",
             "|---|---|---|---|---|---|---|---|"]
    for r in out["calls"]:
        m, q = r["median_ms"], r["quartiles_ms"]
        cell = lambda k: f"{m[k]:.3f} [{q[k][0]:.3f}, {q[k][1]:.3f}]"
        lines.append(f"| {r['case']} | {cell('ours')} | {cell('torch_a')} | {cell('torch_b')} | {r['ours_over_torch']:.2f} | "
                     f"{r['ours_bytes_per_s'] / 1e9:.0f} | {r['copy_bytes_per_s'] / 1e9:.0f} | {100 * r['share_of_copy_rate']:.1f} % |")
    lines.append("")
    for r in out["calls"]:
        lines.append(f"- {r['case']}: {r['note']}.")
    if out.get("clips"):
        lines += ["", "The unik3d step (`tools/depth_engine_video.py`) on a 300-frame 960x540 clip with a stub model on the device, batches of 16, "
                  "wall clock around the whole step (decode, the three entry points, the stub, the read-back per batch, the sink, encode, the files):", "",
                  "| decoder | encoder | seconds | frames/s |", "|---|---|---|---|"]
        for r in out["clips"]:
            lines.append(f"| {r['decoder']} | {r['encoder']} | {r['seconds']:.2f} | {r['frames_per_s']:.0f} |")
    return "\n".join(lines) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=50, help="timed calls per series and case")
    p.add_argument("--clips", action="store_true", help="also time the unik3d step on a 300-frame clip with a stub model")
    p.add_argument("--json", default=None, help="write all rows to this file")
    p.add_argument("--md", default=None, help="write the rows as a markdown report to this file")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_engines_bench needs a GPU: a timing taken elsewhere says nothing about it")
    out = dict(calls=bench_calls(args))
    if args.clips:
        out["clips"] = bench_clips(args)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(markdown(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
