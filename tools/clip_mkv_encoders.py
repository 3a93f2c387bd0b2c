"""The CLI from .mkv to .mkv with each --video_encoder: the product default (mesh, --infill_mask, convergence) on a synthetic 1080p
clip, frames/s including all host I/O, and a byte comparison of every output file of the two runs.  With --decoders the four
--video_decoder x --video_encoder combinations run, each followed by basic_nomal_infill on its outputs with the same decoder
(the two-step chain on .mkv files), and every file is compared with the all-host run's.

--input-class golomb-gop12 writes the two inputs in the class FFmpeg writes by default (Golomb-Rice, a key frame every 12 frames);
the device decoder of the --decoders axis is then --video_decoder device_all.  Every row names its input class.

    python tools/clip_mkv_encoders.py [--frames 300] [--width 1920] [--height 1080] [--batch 16] [--dir DIR] [--json out.json]
                                      [--decoders] [--input-class intra|golomb-gop12]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--decoders", action="store_true", help="also the --video_decoder axis and the basic_nomal_infill step")
    ap.add_argument("--input-class", default="intra", choices=("intra", "golomb-gop12"),
                    help="the stream class of the two input videos: this project's writer's (default) or FFmpeg's default")
    a = ap.parse_args(argv)
    cls = dict(coder=0, gop=12) if a.input_class == "golomb-gop12" else {}
    dev_dec = "device_all" if cls else "device"
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, stereo_rerender as sr, video_io
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    root = a.dir or tempfile.mkdtemp(prefix="clip_mkv_")
    W, H, N = a.width, a.height, a.frames
    dp, cp = os.path.join(root, "in_depth.mkv"), os.path.join(root, "in.mkv")
    sc = SyntheticScene(W, H, config_id=3, n_fg=6)
    with video_io.VideoWriter(dp, W, H, 30.0, bgr=True, **cls) as wd, video_io.VideoWriter(cp, W, H, 30.0, bgr=True, **cls) as wc:
        for t in range(N):
            d, c = sc.frame(t)
            wd.write(np.ascontiguousarray(d[..., ::-1]))
            wc.write(np.ascontiguousarray(c[..., ::-1]))
    conv = os.path.join(root, "conv.json")
    with open(conv, "w") as f:
        json.dump([2.5 + 0.01 * (k % 50) for k in range(N)], f)
    res, files = {}, {}
    combos = [("host", e) for e in ("host", "device")] + ([(dev_dec, e) for e in ("host", "device")] if a.decoders else [])
    for dec, enc in combos:
        name = enc if dec == "host" else f"{dec}_decoder_{enc}"
        d = os.path.join(root, name)
        os.makedirs(d, exist_ok=True)
        for src in (dp, cp):
            dst = os.path.join(d, os.path.basename(src))
            if not os.path.exists(dst):
                os.link(src, dst) if os.stat(src).st_dev == os.stat(d).st_dev else shutil.copy(src, dst)
        t0 = time.perf_counter()
        sr.main(["--depth_video", os.path.join(d, "in_depth.mkv"), "--color_video", os.path.join(d, "in.mkv"), "--xfov", "50",
                 "--pupillary_distance", "65", "--infill_mask", "--convergence_file", conv, "--batch", str(a.batch),
                 "--video_encoder", enc] + (["--video_decoder", dec] if a.decoders else []))
        dt = time.perf_counter() - t0
        dt2 = None
        if a.decoders:
            t0 = time.perf_counter()
            bni.main(["--sbs_color_video", os.path.join(d, "in_depth.mkv_stereo.mkv"), "--sbs_mask_video",
                      os.path.join(d, "in_depth.mkv_stereo.mkv_infillmask.mkv"), "--batch", str(a.batch), "--video_decoder", dec,
                      "--video_encoder", enc])
            dt2 = time.perf_counter() - t0
        outs = sorted(f for f in os.listdir(d) if f.startswith("in_depth.mkv_"))
        files[name] = {f: os.path.getsize(os.path.join(d, f)) for f in outs}
        res[name] = dict(input_class=a.input_class, decoder=dec, encoder=enc, seconds=dt, fps=N / dt, outputs=files[name])
        print(f"class {a.input_class:>12} decoder {dec:>10} encoder {enc:>6}: {N} frames in {dt:.2f} s = {N / dt:.1f} frames/s (whole CLI call, incl. start-up), "
              f"outputs {files[name]}", flush=True)
        if dt2 is not None:
            res[name].update(infill_seconds=dt2, infill_fps=N / dt2)
            print(f"        basic_nomal_infill on them: {dt2:.2f} s = {N / dt2:.1f} frames/s", flush=True)
    same = all(files["host"].keys() == files[k].keys() and
               all(open(os.path.join(root, "host", f), "rb").read() == open(os.path.join(root, k, f), "rb").read() for f in files["host"])
               for k in files if k != "host")
    res["identical"] = bool(same)
    print("outputs byte-identical:", same)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    if not a.dir:
        shutil.rmtree(root)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
