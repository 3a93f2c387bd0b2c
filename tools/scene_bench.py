#!/usr/bin/env python3
"""Times mdvt_scene_frame_sums (include/mdvt_scene.h) on the GPU next to its yardsticks on the same box, in the same process:

    python tools/scene_bench.py [--calls 50] [--clips] [--json out.json] [--md profiles/r24_scene_detect.md]
    python tools/scene_bench.py --once 1|7          one call per factor and nothing else (for tools/pmc_traffic_cmd.sh)

The calls alternate, one of each per round, so every series sees the same box; medians of --calls calls with quartiles, timed by
device events.  There is no pass mark on speed: nothing had been measured before, so nothing is gated.

  factor 1   the sums of 128 x 1920x1080 (127 pairs), next to a device-to-device copy of the same frames' bytes -- the copy rate is
             the yardstick: the kernel reads every byte once and writes nothing to speak of, the copy reads and writes them -- and
             next to the obvious torch composition on the device (integer HSV by the header's formula with table look-ups, 16 frames
             at a time, absolute differences, sums)
  factor 7   the same frames at --downscale auto's factor (274 x 154), next to the same copy and to torch's composition behind
             F.interpolate(bilinear) -- other bits than cv2's 8-bit resize, the same work

--clips: a 300-frame 960x540 clip through tools/scene_detect.py with the host and the device decoder.
Nothing here runs without a GPU."""
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

N, W, H = 128, 1920, 1080


def _tool():
    spec = importlib.util.spec_from_file_location("scene_detect_tool", os.path.join(REPO, "tools", "scene_detect.py"))
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


def _series(torch, fns, calls):
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            t[k].append(_timed(torch, fn))
    return {k: dict(median_ms=float(np.median(v)), quartiles_ms=[float(np.percentile(v, 25)), float(np.percentile(v, 75))]) for k, v in t.items()}


def _tables(torch):
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.concatenate([[0], np.rint((255 << 12) / i)]).astype(np.int32)
    hdiv = np.concatenate([[0], np.rint((180 << 12) / (6.0 * i))]).astype(np.int32)
    return torch.from_numpy(sdiv).cuda(), torch.from_numpy(hdiv).cuda()


def torch_hsv(torch, frames, sdiv, hdiv):
    """uint8 [n, h, w, 3] -> int32 H, S, V by the header's formula."""
    c = frames.to(torch.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = torch.maximum(r, torch.maximum(g, b))
    d = v - torch.minimum(r, torch.minimum(g, b))
    s = torch.clamp_max((d * sdiv[v] + 2048) >> 12, 255)
    h = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * d, r - g + 4 * d))
    hh = (h * hdiv[d] + 2048) >> 12
    return torch.where(hh < 0, hh + 180, hh), s, v


def torch_sums(torch, frames, sdiv, hdiv, size=None, chunk=16):
    """The obvious composition: [pairs, 3] int64."""
    import torch.nn.functional as nnf
    out, last = [], None
    for a in range(0, frames.shape[0], chunk):
        f = frames[a:a + chunk]
        if size is not None:
            f = nnf.interpolate(f.permute(0, 3, 1, 2).float(), size=size, mode="bilinear", align_corners=False).round().clamp(0, 255)
            f = f.to(torch.uint8).permute(0, 2, 3, 1)
        hsv = torch.stack(torch_hsv(torch, f, sdiv, hdiv), dim=1)                  # [n, 3, h, w]
        if last is not None:
            hsv = torch.cat([last, hsv])
        out.append((hsv[1:] - hsv[:-1]).abs().sum(dim=(2, 3), dtype=torch.int64))
        last = hsv[-1:]
    return torch.cat(out)


def _setup():
    import torch
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    g = torch.Generator(device="cuda").manual_seed(24)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    sums = torch.empty((N - 1, 3), dtype=torch.int64, device="cuda")
    stream = _lib.stream_arg(torch.device("cuda", 0))

    def ours(factor):
        ctx.check(L.mdvt_scene_frame_sums(ctx.handle, W, H, N, frames.data_ptr(), 3 * W, 3 * W * H, 0, None, 0, factor, sums.data_ptr(), stream))
    return torch, L, ctx, frames, sums, ours


def bench_calls(args):
    torch, L, ctx, frames, sums, ours = _setup()
    rows = []
    try:
        sdiv, hdiv = _tables(torch)
        frames_copy = torch.empty_like(frames)
        mb = N * W * H * 3 / 1e6
        for factor in (1, 7):
            aw, ah = round(W / factor), round(H / factor)
            size = None if factor == 1 else (ah, aw)
            assert L.mdvt_scene_vector_path(N, frames.data_ptr(), 3 * W, 3 * W * H, None, 0, factor) == (factor == 1)
            ours(factor)
            same = bool(torch.equal(torch_sums(torch, frames, sdiv, hdiv, size), sums)) if factor == 1 else None
            r = _series(torch, {"mdvt_scene_frame_sums": lambda: ours(factor),
                                "device copy of the frames' bytes": lambda: frames_copy.copy_(frames),
                                "torch composition (integer HSV, 16 frames at a time)": lambda: torch_sums(torch, frames, sdiv, hdiv, size)}, args.calls)
            t, tc = r["mdvt_scene_frame_sums"]["median_ms"], r["device copy of the frames' bytes"]["median_ms"]
            copy = f"the copy moves them at {mb / tc / 1e3:.2f} TB/s (read and written: {2 * mb / tc / 1e3:.2f} TB/s of traffic)"
            if factor == 1:
                note = (f"the frames are {mb:.0f} MB: {mb / t / 1e3:.2f} TB/s of input read once, {copy}; achieved fraction of the copy rate "
                        f"{tc / t:.2f}; sums equal to torch's composition on the device: {same}")
            else:
                note = (f"the frames are {mb:.0f} MB, {copy}; the call takes {t / tc:.2f} of the copy's time, but it does not read the frames in full: "
                        f"analysed image {aw} x {ah}, the gathers touch about 2 of every {factor} rows (the bytes read are under HBM traffic); "
                        "torch's resize has other bits, its sums are not compared")
            rows.append(dict(case=f"factor {factor}: {N} x {W}x{H}, {N - 1} pairs", series=r, calls=args.calls, note=note))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        ctx.close()
    return rows


def once(factor):
    torch, L, ctx, frames, sums, ours = _setup()
    try:
        ours(int(factor))
        torch.cuda.synchronize()
    finally:
        ctx.close()
    print(f"one call, factor {factor}: algorithmic bytes {N * W * H * 3 / 1e6:.2f} MB read (each frame once), {(N - 1) * 24} B written")


def bench_clips(args):
    import torch
    from metric_depth_video_toolbox_amd import scene_detect as host, video_io
    tool = _tool()
    w, h, n = 960, 540, 300
    rows = []
    with tempfile.TemporaryDirectory() as d:
        base = np.random.default_rng(n).integers(0, 256, (h, w, 3), dtype=np.uint8)
        clip = os.path.join(d, f"clip{n}.mkv")
        with video_io.VideoWriter(clip, w, h, 24.0) as wr:
            for k in range(n):
                wr.write(np.roll(base, 3 * k + (k // 100) * 400, axis=1))
        tool.run_clip(host.build_parser().parse_args(["--color_video", clip, "--output", os.path.join(d, "warm.csv")]))      # warms the process
        for dec in ("host", "device"):
            a = host.build_parser().parse_args(["--color_video", clip, "--video_decoder", dec, "--output", os.path.join(d, dec + ".csv")])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, scenes = tool.run_clip(a)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            rows.append(dict(frames=n, size=[w, h], decoder=dec, seconds=s, frames_per_s=n / s, scenes=len(scenes)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def markdown(out):
    calls = out["calls"][0]["calls"]
    lines = ["# r24: scene detection's frame difference sums next to their yardsticks", "",
             f"Written by `tools/scene_bench.py --clips --md` on an MI355X.  Milliseconds are medians of {calls} calls (quartiles in brackets), timed "
             "by device events; the calls of a case alternate in one process.  Nothing had been measured before this step, so nothing is "
             "gated: there is no pass mark on speed.", ""]
    for r in out["calls"]:
        first = next(iter(r["series"].values()))["median_ms"]
        lines += [f"## {r['case']}", "", "| call | ms | over the entry point |", "|---|---|---|"]
        for name, s in r["series"].items():
            lines.append(f"| {name} | {s['median_ms']:.3f} [{s['quartiles_ms'][0]:.3f}, {s['quartiles_ms'][1]:.3f}] | {s['median_ms'] / first:.2f} |")
        lines += ["", f"{r['note']}.", ""]
    if out.get("clips"):
        lines += ["## The tool", "", "`tools/scene_detect.py` on a 300-frame 960x540 clip (`--downscale auto`: factor 3; batches of 64), wall clock around "
                  "the whole step (decode, the sums, 24 bytes per pair read back, the detector, the file):", "",
                  "| decoder | seconds | frames/s | scenes |", "|---|---|---|---|"]
        for r in out["clips"]:
            lines.append(f"| {r['decoder']} | {r['seconds']:.2f} | {r['frames_per_s']:.0f} | {r['scenes']} |")
        lines.append("")
    if out.get("traffic"):
        lines += ["## HBM traffic", "", out["traffic"], ""]
    return "\n".join(lines) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=50, help="timed calls per series and case")
    p.add_argument("--clips", action="store_true", help="also time tools/scene_detect.py on a 300-frame clip")
    p.add_argument("--once", default=None, help="one call at this factor and nothing else (for a counters-only run)")
    p.add_argument("--traffic", default=None, help="a text file whose content goes under 'HBM traffic' in the report")
    p.add_argument("--json", default=None, help="write all rows to this file")
    p.add_argument("--md", default=None, help="write the rows as a markdown report to this file")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench needs a GPU: a timing taken elsewhere says nothing about it")
    if args.once is not None:
        once(args.once)
        return 0
    out = dict(calls=bench_calls(args))
    if args.clips:
        out["clips"] = bench_clips(args)
    if args.traffic:
        with open(args.traffic) as fh:
            out["traffic"] = fh.read().strip()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(markdown(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
