#!/usr/bin/env python3
"""Times the three entry points of include/mdvt_mvsa.h on the GPU next to their yardsticks on the same box, in the same process:

    python tools/mvsa_bench.py [--calls 50] [--clips] [--json out.json] [--md out.md]

The yardsticks are torch's own compositions and this library's existing calls, never the code under test.  The calls alternate, one
of each per round, so every series sees the same box; medians of --calls calls with quartiles, timed by device events.  There is no
pass mark on speed: nothing had been measured before, so nothing is gated.

  input    16 x 1920x1080 -> 1024x576 through mdvt_bilinear_model_frames, next to torch's composition on the device (permute,
           .float() / 255, F.interpolate(bilinear)), the existing mdvt_model_frames at the same sizes (cv2's 8-bit resize: other
           bits, the same traffic) and a device copy of the frames' bytes
  output   16 planes 1024x576 -> (512x288) -> 1920x1080 through mdvt_nearest_depth_codes, next to torch's two F.interpolate(nearest)
           followed by mdvt_depth_video_codes at equal size
  median   16 x 512x288 through mdvt_ratio_median, next to torch.median on the device, frame by frame as the reference does it

--clips: the step on a 300-frame 960x540 clip through tools/video_mvsa.py with a stub model, with host and with device codecs.
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


def _tool():
    spec = importlib.util.spec_from_file_location("video_mvsa_tool", os.path.join(REPO, "tools", "video_mvsa.py"))
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


def bench_calls(args):
    import torch
    import torch.nn.functional as nnf
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    dev = torch.device("cuda", 0)
    stream = _lib.stream_arg(dev)
    rows = []
    try:
        g = torch.Generator(device="cuda").manual_seed(20)
        n, (W, H), (w, h) = 16, (1920, 1080), (1024, 576)
        # ---- input
        frames = torch.randint(0, 256, (n, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
        out_cv = torch.empty_like(out)
        frames_copy = torch.empty_like(frames)

        def ours():
            ctx.check(L.mdvt_bilinear_model_frames(ctx.handle, W, H, n, frames.data_ptr(), 3 * W, 3 * W * H, 0, w, h, out.data_ptr(), 4 * w,
                                                   4 * w * h, 12 * w * h, stream))

        def existing():
            ctx.check(L.mdvt_model_frames(ctx.handle, W, H, n, frames.data_ptr(), 3 * W, 3 * W * H, 0, w, h, 1, out_cv.data_ptr(), 4 * w, 4 * w * h,
                                          12 * w * h, stream))
        yard = lambda: nnf.interpolate(frames.permute(0, 3, 1, 2).float() / 255.0, size=(h, w), mode="bilinear", align_corners=False)
        ours()
        close = float((yard() - out).abs().max())
        r = _series(torch, {"mdvt_bilinear_model_frames": ours, "torch permute, float / 255, interpolate": yard, "mdvt_model_frames (cv2's u8 resize)": existing,
                            "device copy of the frames' bytes": lambda: frames_copy.copy_(frames)}, args.calls)
        rows.append(dict(case=f"input {n} x {W}x{H} -> {w}x{h}", series=r, calls=args.calls,
                         note=f"largest difference to torch's result on the device {close:.3g}; the frames are {n * W * H * 3 / 1e6:.0f} MB, the planes "
                              f"{n * w * h * 12 / 1e6:.0f} MB"))
        print(json.dumps(rows[-1]), flush=True)
        # ---- output
        depth = torch.rand((n, h, w), generator=g, device="cuda") * 120.0
        codes = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        codes_t = torch.empty_like(codes)
        mw, mh = 512, 288

        def ours_o():
            ctx.check(L.mdvt_nearest_depth_codes(ctx.handle, w, h, n, depth.data_ptr(), 4 * w, 4 * w * h, mw, mh, None, 0, 100.0, W, H,
                                                 codes.data_ptr(), 3 * W, 3 * W * H, 0, None, 0, 0, stream))

        def yard_o():
            full = nnf.interpolate(nnf.interpolate(depth[:, None], size=(mh, mw), mode="nearest"), size=(H, W), mode="nearest")[:, 0]
            ctx.check(L.mdvt_depth_video_codes(ctx.handle, W, H, n, full.data_ptr(), 4 * W, 4 * W * H, None, 0, 100.0, W, H, codes_t.data_ptr(), 3 * W,
                                               3 * W * H, 0, None, 0, 0, stream))
        ours_o()
        yard_o()
        same = bool(torch.equal(codes, codes_t))
        r = _series(torch, {"mdvt_nearest_depth_codes": ours_o, "torch's two interpolate(nearest), then mdvt_depth_video_codes": yard_o}, args.calls)
        rows.append(dict(case=f"output {n} x {w}x{h} -> {mw}x{mh} -> {W}x{H}", series=r, calls=args.calls,
                         note=f"codes equal to the composition's on the device: {same}; the codes are {n * W * H * 3 / 1e6:.0f} MB"))
        print(json.dumps(rows[-1]), flush=True)
        # ---- median
        cv = torch.rand((n, mh, mw), generator=g, device="cuda") * 50.0 - 2.0
        ref = torch.rand((n, h, w), generator=g, device="cuda") * 50.0 + 0.1
        mask = (torch.rand((n, mh, mw), generator=g, device="cuda") < 0.7).to(torch.uint8)
        med = torch.empty((n,), dtype=torch.float32, device="cuda")

        def ours_m():
            ctx.check(L.mdvt_ratio_median(ctx.handle, n, mw, mh, cv.data_ptr(), 4 * mw, 4 * mw * mh, w, h, ref.data_ptr(), 4 * w, 4 * w * h,
                                          mw, mh, mask.data_ptr(), mw, mw * mh, med.data_ptr(), None, stream))

        def yard_m():
            res = []
            for k in range(n):                                      # video_mvsa.py:261-293 per frame, without the .item()
                d_cv, m = cv[k][None, None], mask[k][None, None].bool()
                d_ref = nnf.interpolate(ref[k][None, None], size=(mh, mw), mode="nearest")
                valid = m & torch.isfinite(d_cv) & torch.isfinite(d_ref) & (d_cv > 0) & (d_ref > 0)
                res.append((d_cv[valid] / (d_ref[valid] + 1e-6)).clamp_min(0.0).median())
            return torch.stack(res)
        ours_m()
        same = bool(torch.equal(yard_m(), med))
        r = _series(torch, {"mdvt_ratio_median": ours_m, "torch.median per frame": yard_m}, args.calls)
        rows.append(dict(case=f"median {n} x {mw}x{mh} (refined depth {w}x{h}, mask {mw}x{mh})", series=r, calls=args.calls,
                         note=f"medians equal to torch's on the device, bit for bit: {same}; torch's boolean indexing synchronises the host once per "
                              "frame inside the window: that is its cost"))
        print(json.dumps(rows[-1]), flush=True)
    finally:
        ctx.close()
    return rows


def stub_model(cur_data, src_data, fast_cost_volume):
    """A stand-in for the model, on the device: the refined depth from the target's red plane, the cost volume's depth at half
    resolution from the first reference's green plane, a mask from its blue plane."""
    image, refs = cur_data["image_b3hw"], src_data["image_b3hw"]
    return {"depth_pred_s0_b1hw": image[:, :1] * 24.0 + 0.5, "lowest_cost_bhw": refs[:, 0, 1, ::2, ::2] * 30.0 + 0.25,
            "overall_mask_bhw": refs[:, 0, 2, ::2, ::2] > 0.3}


def bench_clips(args):
    import torch
    from metric_depth_video_toolbox_amd import video_io, video_mvsa
    tool = _tool()
    W, H, n = 960, 540, 300
    rows = []
    with tempfile.TemporaryDirectory() as d:
        base = np.random.default_rng(n).integers(0, 256, (H, W, 3), dtype=np.uint8)
        clip = os.path.join(d, f"clip{n}.mkv")
        with video_io.VideoWriter(clip, W, H, 24.0) as wr:
            for k in range(n):
                wr.write(np.roll(base, 3 * k, axis=1))
        common = ["--color_video", clip, "--xfov", "60", "--batch", "16", "--apply_cost_volume_scale", "--save_cost_volume_scales"]
        tool.run(video_mvsa.build_parser().parse_args(common + ["--max_frames", "32"]), stub_model)      # the first run warms the process
        for dec, enc in (("host", "host"), ("device", "device")):
            a = video_mvsa.build_parser().parse_args(common + ["--video_decoder", dec, "--video_encoder", enc])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tool.run(a, stub_model)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            rows.append(dict(frames=n, size=[W, H], decoder=dec, encoder=enc, seconds=s, frames_per_s=n / s))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def markdown(out):
    calls = out["calls"][0]["calls"]
    lines = ["# r20: the MVSAnywhere step's entry points next to their yardsticks", "",
             f"Written by `tools/mvsa_bench.py --clips --md` on an MI355X.  Milliseconds are medians of {calls} calls (quartiles in brackets), timed "
             "by device events; the calls of a case alternate in one process.  Nothing had been measured before this step, so nothing is "
             "gated: there is no pass mark on speed.", ""]
    for r in out["calls"]:
        first = next(iter(r["series"].values()))["median_ms"]
        lines += [f"## {r['case']}", "", "| call | ms | over the entry point |", "|---|---|---|"]
        for name, s in r["series"].items():
            lines.append(f"| {name} | {s['median_ms']:.3f} [{s['quartiles_ms'][0]:.3f}, {s['quartiles_ms'][1]:.3f}] | {s['median_ms'] / first:.2f} |")
        lines += ["", f"{r['note']}.", ""]
    if out.get("clips"):
        lines += ["## The tool", "", "`tools/video_mvsa.py` on a 300-frame 960x540 clip (model size 1024x576, window 7, batches of 16) with a stub model on the "
                  "device, the median computed and applied, wall clock around the whole step (decode, the resize, the dicts, the stub, the median, "
                  "the codes, encode, the files):", "", "| decoder | encoder | seconds | frames/s |", "|---|---|---|---|"]
        for r in out["clips"]:
            lines.append(f"| {r['decoder']} | {r['encoder']} | {r['seconds']:.2f} | {r['frames_per_s']:.0f} |")
    return "\n".join(lines) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=50, help="timed calls per series and case")
    p.add_argument("--clips", action="store_true", help="also time the step on a 300-frame clip with a stub model")
    p.add_argument("--json", default=None, help="write all rows to this file")
    p.add_argument("--md", default=None, help="write the rows as a markdown report to this file")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mvsa_bench needs a GPU: a timing taken elsewhere says nothing about it")
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
