#!/usr/bin/env python3
"""Times mdvt_masked_shift_grid (include/mdvt_inspatio.h) on the GPU next to its yardsticks on the same box, in the same process:

    python tools/inspatio_bench.py [--calls 50] [--frames 16] [--clips] [--json out.json]

  shift grid   16 eyes of 960 x 1080 (cells of 270 x 240, the transform path), next to
               - the same six integer sums of the 8 interior cells per frame made with torch.fft.rfft2 in float64 plus round on the
                 device, the obvious composition (five spectra, six products, six inverse transforms; it stops at the sums: no formula,
                 no maxima, no border columns), and
               - a device-to-device copy of the frames' bytes (render, infilled frame, validity plane).

The calls alternate, one of each per round, so every series sees the same box; medians of --calls calls with quartiles, timed by
device events.  There is no pass mark on speed: nothing had been measured before, so nothing is gated.

  warp         mdvt_flow_warp on the same 16 eyes with random grids, next to a device copy of the frames it reads
  prepare      mdvt_inspatio_prepare_eye on 16 side-by-side frames of 1920 x 1080 -> 832 x 480, next to a copy of the eye's halves

  composite    mdvt_inspatio_composite_eye with blending on the same 16 frames, next to a copy of the eye's halves of its inputs

--clips: a 300-frame clip of 960 x 540 side-by-side frames through tools/inspatio_world_infill.py with a stub generator on the device
(it returns the render it was handed), blending on, with host and with device codecs.  Nothing here runs without a GPU."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY = "device copy of the input bytes"
TORCH = "torch.fft.rfft2 in float64 + round: the six sums of the interior cells"


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


def torch_sums(torch, render, infilled, valid):
    """The six sums of every interior cell, [6, n * 8, 2 h - 1, 2 w - 1] int64 (displacement d at index d mod the transform's size is
    left where the inverse transform puts it: the yardstick does not pay for the reordering)."""
    n, H, W, _ = render.shape
    h, w = H // 4, W // 4
    assert H % 4 == 0 and W % 4 == 0

    def grey(f):
        f = f.int()
        return (4899 * f[..., 0] + 9617 * f[..., 1] + 1868 * f[..., 2] + 8192) >> 14

    def cells(p):                                                   # [n, H, W] -> the interior cells [n * 8, h, w]
        return p.reshape(n, 4, h, 4, w)[:, :, :, 1:3].permute(0, 1, 3, 2, 4).reshape(n * 8, h, w)
    v = cells((valid != 0).double())
    a, b = cells(grey(infilled).double()) * v, cells(grey(render).double()) * v
    size = (2 * h, 2 * w)
    fv, fa, fb, fa2, fb2 = (torch.fft.rfft2(x, s=size) for x in (v, a, b, a * a, b * b))
    pairs = ((fv, fv), (fa, fv), (fv, fb), (fa, fb), (fa2, fv), (fv, fb2))
    return torch.stack([torch.fft.irfft2(x * y.conj(), s=size).round().long() for x, y in pairs])


def stub_generator(source, render, mask, fps, text_prompt):
    return render.clone()


def bench_clips(torch, n=300, W2=960, H=540):
    import importlib.util
    import tempfile
    import time
    from metric_depth_video_toolbox_amd import video_io
    spec = importlib.util.spec_from_file_location("inspatio_world_infill_tool", os.path.join(REPO, "tools", "inspatio_world_infill.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(26)
    base = rng.integers(0, 256, (H, W2, 3), dtype=np.uint8)
    rows = {}
    with tempfile.TemporaryDirectory() as d:
        paths = {k: os.path.join(d, k + ".mkv") for k in ("sbs", "mask", "org")}
        writers = {k: video_io.VideoWriter(paths[k], W2 if k != "org" else W2 // 2, H, 25.0) for k in paths}
        for t in range(n):
            frame = np.roll(base, 3 * t, axis=1)
            mask = np.zeros_like(frame)
            mask[100:160, (40 + 2 * t) % 400:(40 + 2 * t) % 400 + 30] = 255
            mask[300:330, W2 // 2 + 100:W2 // 2 + 180] = 255
            writers["sbs"].write(frame)
            writers["mask"].write(mask)
            writers["org"].write(np.ascontiguousarray(frame[:, :W2 // 2]))
        for w in writers.values():
            w.close()
        for codec in ("host", "device"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            final = tool.process_pair(paths["sbs"], paths["mask"], paths["org"], stub_generator, apply_edge_blending=True,
                                      video_decoder=codec, video_encoder=codec)
            torch.cuda.synchronize()
            rows[codec] = dict(seconds=time.perf_counter() - t0, frames_per_s=n / (time.perf_counter() - t0))
            os.remove(final)
    return dict(case=f"{n} frames of {W2}x{H} through tools/inspatio_world_infill.py, stub generator, blending on", codecs=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--clips", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from metric_depth_video_toolbox_amd import _lib, inspatio_device as idev
    ctx = _lib.Context(0, 16, 16)
    try:
        g = torch.Generator(device="cuda").manual_seed(26)
        n, H, W = args.frames, 1080, 960
        valid = (torch.rand((n, H, W), generator=g, device="cuda") < 0.8).to(torch.uint8) * 255
        render = torch.randint(0, 256, (n, H, W, 3), generator=g, device="cuda", dtype=torch.uint8) * (valid != 0)[..., None]
        infilled = torch.roll(render, (-4, 6), dims=(1, 2))
        copies = [torch.empty_like(t) for t in (render, infilled, valid)]

        def copy():
            for dst, src in zip(copies, (render, infilled, valid)):
                dst.copy_(src)
        shift, status, err = idev.masked_shift_grid(ctx, render, infilled, valid)
        torch.cuda.synchronize()
        found = shift[:, :, 1:3].reshape(-1, 2)
        ok = bool((found == torch.tensor([4.0, -6.0], dtype=torch.float64, device="cuda")).all()) and bool(status.all())
        sums = torch_sums(torch, render[:1], infilled[:1], valid[:1])
        n_valid = (valid[0].reshape(4, H // 4, 4, W // 4)[:, :, 1:3] != 0).sum(dim=(1, 3)).reshape(-1)
        ok_torch = bool((sums[0, :, 0, 0] == n_valid).all())       # N at displacement 0 is the cell's valid pixels
        r = _series(torch, {"mdvt_masked_shift_grid": lambda: idev.masked_shift_grid(ctx, render, infilled, valid), TORCH: lambda: torch_sums(torch, render, infilled, valid),
                            COPY: copy}, args.calls)
        twice = _series(torch, {"first": lambda: torch_sums(torch, render, infilled, valid), "second": lambda: torch_sums(torch, render, infilled, valid)}, max(4, args.calls // 5))
        out = dict(case=f"shift grid {n} x {W}x{H}, cells of {H // 4} x {W // 4}, path {_lib.load().mdvt_masked_shift_path(W, H)}", series=r, calls=args.calls,
                   input_mb=sum(t.numel() for t in (render, infilled, valid)) / 1e6, every_interior_shift_found=ok, torch_sums_checked=ok_torch,
                   largest_distance_from_an_integer=float(err.cpu()[0]), workspace_mb=ctx.workspace_bytes() / 1e6,
                   yardstick_two_series_ms=[twice["first"]["median_ms"], twice["second"]["median_ms"]],
                   share_of_copy_rate=r[COPY]["median_ms"] / r["mdvt_masked_shift_grid"]["median_ms"])
        print(json.dumps(out), flush=True)
        # ---- the warp and the frame preparation, next to a device copy of what they read
        grids = (torch.rand((n, 4, 4, 2), generator=g, device="cuda") * 8 - 4).contiguous()
        has = torch.ones((n,), dtype=torch.uint8, device="cuda")
        warped = torch.empty_like(infilled)
        inf_copy = torch.empty_like(infilled)
        rw = _series(torch, {"mdvt_flow_warp": lambda: idev.flow_warp(ctx, grids, has, infilled, out=warped), COPY: lambda: inf_copy.copy_(infilled)}, args.calls)
        sbs_c = torch.randint(0, 256, (n, H, 2 * W, 3), generator=g, device="cuda", dtype=torch.uint8)
        sbs_m = ((torch.rand((n, H, 2 * W, 1), generator=g, device="cuda") < 0.2).to(torch.uint8) * 255).expand(n, H, 2 * W, 3).contiguous()
        half_c, half_m = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda"), torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")

        def copy_eye():
            half_c.copy_(sbs_c[:, :, W:])
            half_m.copy_(sbs_m[:, :, W:])
        rp = _series(torch, {"mdvt_inspatio_prepare_eye": lambda: idev.prepare_eye(ctx, sbs_c, sbs_m, 1, (832, 480)), COPY: copy_eye}, args.calls)
        out["warp"] = dict(case=f"flow warp {n} x {W}x{H}", series=rw, share_of_copy_rate=rw[COPY]["median_ms"] / rw["mdvt_flow_warp"]["median_ms"])
        out["prepare"] = dict(case=f"prepare eye {n} x {W}x{H} -> 832x480 (the wrapper allocates its five outputs)", series=rp,
                              share_of_copy_rate=rp[COPY]["median_ms"] / rp["mdvt_inspatio_prepare_eye"]["median_ms"])
        aligned = infilled
        pasted, blended = torch.empty_like(sbs_c), torch.empty_like(sbs_c)
        half_a = torch.empty_like(aligned)

        def copy_comp():
            copy_eye()
            half_a.copy_(aligned)
        rc = _series(torch, {"mdvt_inspatio_composite_eye": lambda: idev.composite_eye(ctx, aligned, sbs_c, sbs_m, 1, pasted, blended), COPY: copy_comp}, args.calls)
        out["composite"] = dict(case=f"composite eye {n} x {W}x{H}, blending on", series=rc,
                                share_of_copy_rate=rc[COPY]["median_ms"] / rc["mdvt_inspatio_composite_eye"]["median_ms"])
        print(json.dumps(out["composite"]), flush=True)
        if args.clips:
            out["clips"] = bench_clips(torch)
            print(json.dumps(out["clips"]), flush=True)
        print(json.dumps(out["warp"]), flush=True)
        print(json.dumps(out["prepare"]), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
