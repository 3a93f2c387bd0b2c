#!/usr/bin/env python3
"""Times mdvt_depth_video_codes (include/mdvt_depth_sink.h) on the GPU next to a yardstick, mdvt_metric_depth_codes (style 0) of a
library built from the commit before the sink, in the same process:

    python tools/depth_sink_bench.py [--yardstick-lib path/to/libmdvt_hip.so] [--calls 50] [--clips] [--json out.json]

Three shapes: 128 planes of 924x518 kept at their size, 128 planes of 924x518 -> 1920x1080, 40 planes of 504x280 -> 1920x1080.  The
calls alternate -- yardstick, sink, yardstick again -- so the two yardstick series, the same code on the same box, give the box's
spread; the sink passes if it is not slower than the yardstick by more than that.  Per shape also the bytes the algorithm moves (4 B
per source value, 3 B per code) over the sink's time, against the 6.29 TB/s a float4 copy reaches on the MI355X, and the time NumPy
takes for the restatement (tests/depth_sink_ref.py) on the same box.  Without --yardstick-lib the yardstick is the loaded library's
own mdvt_metric_depth_codes.

--clips: also a 23-frame and a 300-frame 960x540 clip through tools/video_da3.py with a stub model, per decoder and encoder.
Device events time the calls; nothing here runs without a GPU."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = [(128, (924, 518), (924, 518)), (128, (924, 518), (1920, 1080)), (40, (504, 280), (1920, 1080))]
COPY_PEAK = 6.29e12                                      # bytes/s of a float4 copy on the MI355X


def _tool():
    spec = importlib.util.spec_from_file_location("video_da3_tool", os.path.join(REPO, "tools", "video_da3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Yardstick:
    """mdvt_metric_depth_codes of another build of the library, with a context of its own."""

    def __init__(self, path, _lib):
        self.L = C.CDLL(path)
        vp = C.c_void_p
        self.L.mdvt_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_uint32]
        self.L.mdvt_destroy.argtypes = [vp]
        self.L.mdvt_metric_depth_codes.argtypes = _lib.load().mdvt_metric_depth_codes.argtypes
        self.h = vp()
        if self.L.mdvt_create(C.byref(self.h), 0, 16, 16, 0) != 0:
            raise RuntimeError(f"{path}: mdvt_create failed")

    def codes(self, x, ss, max_depth, W, H, out, stream):
        N, h, w = x.shape
        rc = self.L.mdvt_metric_depth_codes(self.h, w, h, N, x.data_ptr(), 4 * x.stride(1), 4 * x.stride(0), ss.data_ptr(), 0, float(max_depth),
                                            W, H, out.data_ptr(), out.stride(1), out.stride(0), 0, None, 0, 0, stream)
        if rc != 0:
            raise RuntimeError(f"the yardstick's mdvt_metric_depth_codes returned {rc}")

    def close(self):
        self.L.mdvt_destroy(self.h)


def _timed(torch, fn, calls):
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def bench_shapes(args):
    import torch
    import depth_sink_ref as dr
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    yard = Yardstick(args.yardstick_lib or _lib.lib_path(), _lib)
    rows = []
    try:
        for N, (w, h), (W, H) in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(N + w)
            depth = torch.rand((N, h, w), generator=g, device="cuda") * 60.0 + 0.5
            rel = 1.0 / depth                                       # the yardstick inverts: the same depths reach its resize and code
            ss = torch.tensor([1.0, 0.0], device="cuda")
            out_s = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
            out_y = torch.empty_like(out_s)
            stream = _lib.stream_arg(depth.device)
            L = _lib.load()

            def sink():                                             # the raw call, as the yardstick's: no Python check inside the timed window
                ctx.check(L.mdvt_depth_video_codes(ctx.handle, w, h, N, depth.data_ptr(), 4 * w, 4 * w * h, None, 0, 100.0, W, H,
                                                   out_s.data_ptr(), 3 * W, 3 * W * H, 0, None, 0, 0, stream))
            yardstick = lambda: yard.codes(rel, ss, 100, W, H, out_y, stream)
            for fn in (sink, yardstick, sink, yardstick):           # every shape is warmed before it is timed
                fn()
            torch.cuda.synchronize()
            t = {"yardstick_a": [], "sink": [], "yardstick_b": []}
            for _ in range(args.calls):
                t["yardstick_a"] += _timed(torch, yardstick, 1)
                t["sink"] += _timed(torch, sink, 1)
                t["yardstick_b"] += _timed(torch, yardstick, 1)
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = abs(med["yardstick_a"] - med["yardstick_b"])
            quartiles = {k: [float(np.percentile(v, 25)), float(np.percentile(v, 75))] for k, v in t.items()}
            moved = N * (4 * w * h + 3 * W * H)
            host = depth[:2].cpu().numpy()
            t0 = time.perf_counter()
            dr.sink(host, 100, (W, H))
            numpy_ms = (time.perf_counter() - t0) / 2 * N * 1e3
            rows.append(dict(planes=N, src=[w, h], out=[W, H], median_ms=med, quartiles_ms=quartiles, yardstick_spread_ms=spread,
                             sink_minus_yardstick_ms=med["sink"] - min(med["yardstick_a"], med["yardstick_b"]),
                             bytes_moved=moved, sink_bytes_per_s=moved / (med["sink"] * 1e-3), share_of_copy_peak=moved / (med["sink"] * 1e-3) / COPY_PEAK,
                             numpy_restatement_ms=numpy_ms, calls=args.calls))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        yard.close()
        ctx.close()
    return rows


def stub_infer(frames, resolution):
    """A stand-in for the model, on the device: a quarter-size depth from the frames' red bytes; the identity pose and a fixed camera."""
    import torch
    depth = frames[:, ::4, ::4, 0].float() / 16.0 + 0.5
    T = int(frames.shape[0])
    ext = np.tile(np.eye(4)[:3][None], (T, 1, 1))
    ext[:, 0, 3] = np.arange(T) * 0.01
    K = np.array([[0.8 * frames.shape[2], 0, frames.shape[2] / 2], [0, 0.8 * frames.shape[2], frames.shape[1] / 2], [0, 0, 1]])
    return depth.contiguous(), ext, np.tile(K[None], (T, 1, 1)).astype(np.float32)


def bench_clips(args):
    import torch
    from metric_depth_video_toolbox_amd import video_da3, video_io
    tool = _tool()
    W, H = 960, 540
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for n in (23, 300):
            rng = np.random.default_rng(n)
            base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            clip = os.path.join(d, f"clip{n}.mkv")
            with video_io.VideoWriter(clip, W, H, 24.0) as wr:
                for k in range(n):
                    wr.write(np.roll(base, 3 * k, axis=1))
            for dec, enc in (("host", "host"), ("device", "host"), ("host", "device"), ("device", "device")):
                a = video_da3.build_parser().parse_args(["--color_video", clip, "--video_decoder", dec, "--video_encoder", enc])
                if n == 23 and (dec, enc) == ("host", "host"):
                    tool.run(a, stub_infer)                         # the first run warms the process
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tool.run(a, stub_infer)
                torch.cuda.synchronize()
                s = time.perf_counter() - t0
                rows.append(dict(frames=n, size=[W, H], decoder=dec, encoder=enc, seconds=s, frames_per_s=n / s))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--yardstick-lib", default=None, help="a libmdvt_hip.so built from the commit before the sink (default: the loaded library itself)")
    p.add_argument("--calls", type=int, default=50, help="timed calls per series and shape")
    p.add_argument("--clips", action="store_true", help="also time clips through tools/video_da3.py with a stub model")
    p.add_argument("--json", default=None, help="write all rows to this file")
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_sink_bench needs a GPU: a timing taken elsewhere says nothing about it")
    out = dict(shapes=bench_shapes(args))
    if args.clips:
        out["clips"] = bench_clips(args)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
