#!/usr/bin/env python3
"""Times the four entry points of include/mdvt_megasam.h on the GPU next to their yardsticks on the same box, in the same process:

    python tools/megasam_bench.py [--calls 50] [--clips] [--json out.json] [--md out.md]

The yardsticks are torch's own compositions on the device and a device-to-device copy of the input bytes, never the code under test.
The calls alternate, one of each per round, so every series sees the same box; medians of --calls calls with quartiles, timed by
device events.  There is no pass mark on speed: nothing had been measured before, so nothing is gated.

  colour   16 x 1920x1080 -> 591x332 -> 584x328 through mdvt_area_model_frames, next to torch's composition (permute, .float(),
           F.interpolate(mode="area"), round, crop: NOT the same bits) and a device copy of the frames' bytes
  depth    16 x 1920x1080 depth frames through mdvt_tracker_depth, next to torch's decode of every pixel, F.interpolate(nearest-exact), crop
  mask     16 x 1920x1080 mask frames through mdvt_tracker_mask, next to torch's grey, F.interpolate(bilinear), crop
  codes    64 planes 73x41 -> 1920x1080 depth codes through mdvt_tracker_outputs mode 0, next to F.interpolate(nearest-exact) followed
           by mdvt_depth_video_codes at equal size
  grey     64 planes 73x41 -> 1920x1080 grey frames through mdvt_tracker_outputs mode 1, next to F.interpolate(bilinear) (not cv2's
           bits), clamp, scale, three bytes

--clips: the step on a 300-frame 960x540 clip through tools/sam_track_video.py with a stub tracker on the device, with host and
with device codecs.  Nothing here runs without a GPU."""
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


def _tool():
    spec = importlib.util.spec_from_file_location("sam_track_video_tool", os.path.join(REPO, "tools", "sam_track_video.py"))
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
    """fns: {name: callable}; every one is warmed twice, then they are timed in turn, `calls` rounds."""
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            t[k].append(_timed(torch, fn))
    return {k: dict(median_ms=float(np.median(v)), quartiles_ms=[float(np.percentile(v, 25)), float(np.percentile(v, 75))]) for k, v in t.items()}


COPY = "device copy of the input bytes"


def bench_calls(args):
    import torch
    import torch.nn.functional as nnf
    from metric_depth_video_toolbox_amd import _lib, megasam_device as md, step_device
    ctx = _lib.Context(0, 16, 16)
    rows = []

    def row(case, fns, note, in_bytes):
        r = _series(torch, fns, args.calls)
        rows.append(dict(case=case, series=r, calls=args.calls, note=note, input_mb=in_bytes / 1e6,
                         share_of_copy_rate=r[COPY]["median_ms"] / next(iter(r.values()))["median_ms"]))
        print(json.dumps(rows[-1]), flush=True)
    try:
        g = torch.Generator(device="cuda").manual_seed(25)
        n, (W, H), mid, crop = 16, (1920, 1080), (591, 332), (584, 328)
        frames = torch.randint(0, 256, (n, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
        frames_copy = torch.empty_like(frames)
        copy = lambda: frames_copy.copy_(frames)
        # ---- colour
        yard = lambda: nnf.interpolate(frames.permute(0, 3, 1, 2).float(), size=(mid[1], mid[0]), mode="area").round().clamp(0, 255).to(torch.uint8)[..., :crop[1], :crop[0]]
        ours = md.area_model_frames(ctx, frames, mid, crop)
        off = (yard().int() - ours.int()).abs()
        row(f"colour {n} x {W}x{H} -> {mid[0]}x{mid[1]} -> {crop[0]}x{crop[1]}",
            {"mdvt_area_model_frames": lambda: md.area_model_frames(ctx, frames, mid, crop),
             "torch permute, float, interpolate(area), round, crop": yard, COPY: copy},
            f"torch's adaptive average pool is another algorithm: {float((off > 0).float().mean()) * 100:.2f} % of the bytes differ, by at most {int(off.max())}",
            frames.numel())
        # ---- depth
        def yard_d():
            u = (frames[..., 0].to(torch.int64) << 24) | (frames[..., 2].to(torch.int64) << 16)
            d = u.float() / float(np.float32(255 ** 4 / 100))
            return nnf.interpolate(d[:, None], size=(mid[1], mid[0]), mode="nearest-exact")[:, 0, :crop[1], :crop[0]]
        same = bool(torch.equal(yard_d(), md.tracker_depth(ctx, frames, 100, mid, crop)))
        row(f"depth {n} x {W}x{H} -> {mid[0]}x{mid[1]} -> {crop[0]}x{crop[1]}",
            {"mdvt_tracker_depth": lambda: md.tracker_depth(ctx, frames, 100, mid, crop), "torch decode, interpolate(nearest-exact), crop": yard_d, COPY: copy},
            f"equal to torch's result on the device, bit for bit: {same}; the call reads only the pixels it takes", frames.numel())
        # ---- mask
        def yard_m():
            f = frames.int()
            grey = (4899 * f[..., 0] + 9617 * f[..., 1] + 1868 * f[..., 2] + 8192) >> 14
            return nnf.interpolate(((255 - grey).float() / 255.0)[:, None], size=(mid[1], mid[0]), mode="bilinear")[:, 0, :crop[1], :crop[0]]
        close = float((yard_m() - md.tracker_mask(ctx, frames, mid, crop)).abs().max())
        row(f"mask {n} x {W}x{H} -> {mid[0]}x{mid[1]} -> {crop[0]}x{crop[1]}",
            {"mdvt_tracker_mask": lambda: md.tracker_mask(ctx, frames, mid, crop), "torch grey, interpolate(bilinear), crop": yard_m, COPY: copy},
            f"largest difference to torch's result on the device {close:.3g}", frames.numel())
        # ---- the outputs
        t, (w, h) = 64, (73, 41)
        planes = torch.rand((t, h, w), generator=g, device="cuda") * 1.2 - 0.1
        out = torch.empty((t, H, W, 3), dtype=torch.uint8, device="cuda")
        out_copy = torch.empty_like(out)
        copy_o = lambda: out_copy.copy_(out)

        def yard_c():
            full = nnf.interpolate(planes[:, None] * 100.0, size=(H, W), mode="nearest-exact")[:, 0]
            return step_device.depth_video_codes(ctx, full, 100.0)
        planes100 = planes * 100.0
        same = bool(torch.equal(yard_c(), md.tracker_outputs(ctx, planes100, 0, 100.0, (W, H))))
        row(f"codes {t} x {w}x{h} -> {W}x{H}",
            {"mdvt_tracker_outputs mode 0": lambda: md.tracker_outputs(ctx, planes100, 0, 100.0, (W, H), out=out),
             "torch interpolate(nearest-exact), then mdvt_depth_video_codes": yard_c, COPY: copy_o},
            f"codes equal to the composition's on the device: {same}; the copy here is of the OUTPUT's bytes ({out.numel() / 1e6:.0f} MB): the input is {planes.numel() * 4 / 1e6:.2f} MB",
            out.numel())

        def yard_g():
            full = nnf.interpolate(planes[:, None], size=(H, W), mode="bilinear")[:, 0]
            return (full.clamp(0, 1) * 255.0).to(torch.uint8)[..., None].expand(-1, -1, -1, 3).contiguous()
        off = (yard_g().int() - md.tracker_outputs(ctx, planes, 1, 1.0, (W, H)).int()).abs()
        row(f"grey {t} x {w}x{h} -> {W}x{H}",
            {"mdvt_tracker_outputs mode 1": lambda: md.tracker_outputs(ctx, planes, 1, 1.0, (W, H), out=out),
             "torch interpolate(bilinear), clamp, * 255, three bytes": yard_g, COPY: copy_o},
            f"torch's bilinear is not cv2's: {float((off > 0).float().mean()) * 100:.2f} % of the bytes differ, by at most {int(off.max())}; the copy "
            "here is of the OUTPUT's bytes", out.numel())
    finally:
        ctx.close()
    return rows


class DeviceStubTracker:
    """A stand-in for the tracker that stays on the device: poses from the frame number, the depth and the motion map from the planes
    it is handed at an eighth of their size."""

    def __init__(self, image_size):
        self.items = []

    def track(self, *item):
        self.items.append(item)

    track_final = track

    def terminate(self, stream, optimize_intrinsic):
        import torch
        dev = self.items[0][1].device
        t = len(self.items)
        i = torch.arange(t, device=dev, dtype=torch.float32)
        a = 0.02 * i
        z = torch.zeros_like(i)
        traj = torch.stack([0.01 * i, -0.02 * i, 0.005 * i * i, z, torch.sin(a / 2), z, torch.cos(a / 2)], dim=1)
        depth = torch.stack([it[2][4::8, 4::8] * 1.25 for it in self.items])
        motion = torch.stack([it[4][4::8, 4::8] * 1.3 - 0.15 + it[1][0, 0, 4::8, 4::8].float() / 255.0 * 0.2 for it in self.items])
        return traj, depth, motion, torch.stack([it[3] / 8 for it in self.items])


def bench_clips(args):
    import torch
    from metric_depth_video_toolbox_amd import sam_track, video_io
    tool = _tool()
    W, H, n = 960, 540, 300
    rows = []
    with tempfile.TemporaryDirectory() as d:
        base = np.random.default_rng(n).integers(0, 256, (H, W, 3), dtype=np.uint8)
        color, depth = os.path.join(d, f"clip{n}.mkv"), os.path.join(d, f"clip{n}.mkv_depth.mkv")
        for path, shift in ((color, 3), (depth, 5)):
            with video_io.VideoWriter(path, W, H, 24.0) as wr:
                for k in range(n + (path == color)):                # the colour video one frame longer: every depth frame is tracked
                    wr.write(np.roll(base, shift * k, axis=1))
        common = ["--color_video", color, "--depth_video", depth, "--xfov", "60", "--batch", "16"]
        tool.run(sam_track.build_parser().parse_args(common + ["--max_frames", "30"]), DeviceStubTracker)      # the first run warms the process
        for dec, enc in (("host", "host"), ("device", "device")):
            a = sam_track.build_parser().parse_args(common + ["--video_decoder", dec, "--video_encoder", enc])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tool.run(a, DeviceStubTracker)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            rows.append(dict(frames=n, size=[W, H], decoder=dec, encoder=enc, seconds=s, frames_per_s=n / s))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def markdown(out):
    calls = out["calls"][0]["calls"]
    lines = ["# r25: the MegaSAM camera-tracking step's entry points next to their yardsticks", "",
             f"Written by `tools/megasam_bench.py --clips --md` on an MI355X.  Milliseconds are medians of {calls} calls (quartiles in brackets), "
             "timed by device events; the calls of a case alternate in one process.  Nothing had been measured before this step, so nothing "
             "is gated: there is no pass mark on speed.  The share of the copy rate is the copy's time over the entry point's: 1.00 would be "
             "a call as fast as a device-to-device copy of the same bytes (which reads and writes them: twice the traffic of a pure read).", ""]
    for r in out["calls"]:
        first = next(iter(r["series"].values()))["median_ms"]
        lines += [f"## {r['case']}", "", "| call | ms | over the entry point |", "|---|---|---|"]
        for name, s in r["series"].items():
            lines.append(f"| {name} | {s['median_ms']:.3f} [{s['quartiles_ms'][0]:.3f}, {s['quartiles_ms'][1]:.3f}] | {s['median_ms'] / first:.2f} |")
        lines += ["", f"{r['note']}.  Copied bytes: {r['input_mb']:.0f} MB; share of the copy rate: {r['share_of_copy_rate']:.2f}.", ""]
    if out.get("clips"):
        lines += ["## The tool", "", "`tools/sam_track_video.py` on a 300-frame 960x540 colour and depth clip (tracker size 584x328, batches of 16) with a stub "
                  "tracker on the device, wall clock around the whole step (two decodes, the three ways in, the stub, the two ways out, two encodes, "
                  "the files):", "", "| decoder | encoder | seconds | frames/s |", "|---|---|---|---|"]
        for r in out["clips"]:
            lines.append(f"| {r['decoder']} | {r['encoder']} | {r['seconds']:.2f} | {r['frames_per_s']:.0f} |")
    return "\n".join(lines) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=50, help="timed calls per series and case")
    p.add_argument("--clips", action="store_true", help="also time the step on a 300-frame clip with a stub tracker")
    p.add_argument("--json", default=None, help="write all rows to this file")
    p.add_argument("--md", default=None, help="write the rows as a markdown report to this file")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("megasam_bench needs a GPU: a timing taken elsewhere says nothing about it")
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
