"""Frames per second of the device FFV1 encoder (ffv1_device.encode_frames_on_device: kernels + packet read-back) against the host
encoder (video_io.encode_frame, 16 threads across frames, one slice thread each: what clip.VideoSink does).

    python tools/ffv1_bench.py [--sizes 1920x1080,3840x1080] [--contents depth,synthetic,noise] [--slices 4x4,8x8]
                               [--frames 16,64,128] [--host-threads 16] [--json out.json]

With --decode the table is the decoder's: ffv1_device.enqueue_decode + the status read-back (packets already packed in pinned host
memory, frames left on the device) against the host decoder as the clip driver uses it (clip.VideoFrames.read_into into pinned memory,
two readers sharing the host threads, + the copy of the raw frames to the device); every timed batch is compared with the host's
bytes first, and the run stops if the device flagged a frame.

--decode --stream-class golomb-gop12 measures mdvt_decode_video_stream on the class FFmpeg writes by default (Golomb-Rice, a key
frame every 12 frames; written here by video_io.VideoWriter(coder=0, gop=12)) against what such a file gets today: one host reader
with --host-threads slice threads + the copy of the raw frames.  The rows carry the class in a `class` field.  --pix-fmt yuv444p /
yuv422p / yuv420p makes the stream YCbCr instead of RGB (tools/ffv1_ycbcr_writer.cpp, compiled here with g++, codes the planes of the
same content; the library itself writes RGB only); the host side is then video_io.StreamDecoder on the packets, --host-threads slice
threads, + the copy, and the rows carry a `pix_fmt` field.

Every device packet is compared with the host's bytes before it is timed, and the run stops if the device flagged any frame
(a flagged frame is re-encoded on the host: its time would not be the device's).  Prints one line per case and, with --json,
writes the table."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frames_of(kind, W, H, n, rng):
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    if kind == "noise":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    sc = SyntheticScene(W, H, config_id=1, n_fg=6)
    out = np.empty((n, H, W, 3), np.uint8)
    for t in range(n):
        d, c = sc.frame(t)
        out[t] = d if kind == "depth" else c
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x1080")
    ap.add_argument("--contents", default="depth,synthetic,noise")
    ap.add_argument("--slices", default="4x4,8x8")
    ap.add_argument("--frames", default="16,64,128")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--decode", action="store_true", help="measure the decoders instead of the encoders")
    ap.add_argument("--stream-class", default="intra", choices=("intra", "golomb-gop12"),
                    help="with --decode: the stream class of the files -- 'intra' (default: this project's writer, mdvt_decode_video_frames) "
                         "or 'golomb-gop12' (Golomb-Rice, a key frame every 12 frames: mdvt_decode_video_stream)")
    ap.add_argument("--pix-fmt", default="rgb", choices=("rgb", "yuv444p", "yuv422p", "yuv420p"),
                    help="with --decode --stream-class golomb-gop12: what the stream codes (default rgb)")
    a = ap.parse_args(argv)
    if a.pix_fmt != "rgb" and not (a.decode and a.stream_class == "golomb-gop12"):
        ap.error("--pix-fmt needs --decode --stream-class golomb-gop12")
    if a.decode:
        return decode_main(a)
    import torch
    from metric_depth_video_toolbox_amd import _lib, ffv1_device, video_io
    rng = np.random.default_rng(1)
    pool = ThreadPoolExecutor(a.host_threads)

    def device(frames, slices):
        p = ffv1_device.enqueue(_lib.shared_context(0), frames, slices=slices)
        pkts = p.collect()
        if p.host_frames:
            raise SystemExit(f"{p.host_frames} of {len(pkts)} frames were flagged by the device and re-encoded on the host "
                             f"({tuple(frames.shape)}, slices {slices}): not a device timing")
        return pkts
    rows = []
    nmax = max(int(v) for v in a.frames.split(","))
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for kind in a.contents.split(","):
            host_frames = frames_of(kind, W, H, nmax, rng)
            dev_frames = torch.from_numpy(host_frames).cuda()
            for sl in a.slices.split(","):
                slices = tuple(int(v) for v in sl.split("x"))
                for n in (int(v) for v in a.frames.split(",")):
                    want = list(pool.map(lambda f: video_io.encode_frame(f, slices=slices, threads=1)[0], host_frames[:n]))
                    got = device(dev_frames[:n], slices)
                    assert got == want, (size, kind, sl, n)
                    dt_dev, dt_host = [], []
                    for _ in range(a.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        device(dev_frames[:n], slices)
                        dt_dev.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        list(pool.map(lambda f: video_io.encode_frame(f, slices=slices, threads=1)[0], host_frames[:n]))
                        dt_host.append(time.perf_counter() - t0)
                    r = dict(size=size, content=kind, slices=sl, frames=n, device_fps=n / min(dt_dev), host_fps=n / min(dt_host),
                             bytes_per_frame=sum(len(p) for p in got) / n)
                    r["speedup"] = r["device_fps"] / r["host_fps"]
                    rows.append(r)
                    print(f"{size:>9} {kind:>9} {sl:>3} n={n:<3} device {r['device_fps']:8.1f} fps  host({a.host_threads}t) "
                          f"{r['host_fps']:8.1f} fps  x{r['speedup']:.2f}  {r['bytes_per_frame'] / 1e6:.2f} MB/frame", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


PIX_SHIFTS = {"yuv444p": (0, 0), "yuv422p": (1, 0), "yuv420p": (1, 1)}


def ycbcr_planes(frames, hs, vs):
    """RGB frames -> (Y, Cb, Cr) per frame: BT.601 limited range in integers, chroma taken at the top left pixel of each block.  Only
    the content of the measured stream: nothing is held to this direction."""
    r, g, b = (frames[..., k].astype(np.int32) for k in range(3))
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    cb = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    cr = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    sub = lambda p: np.ascontiguousarray(p[:, ::1 << vs, ::1 << hs].astype(np.uint8))
    return np.ascontiguousarray(y.astype(np.uint8)), sub(cb), sub(cr)


def ycbcr_stream(frames, pix_fmt, slices, tmp):
    """-> (packets, configuration record) of the frames as a YCbCr stream of the class, by tools/ffv1_ycbcr_writer.cpp"""
    import struct
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(tmp, "ffv1_ycbcr_writer")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wno-subobject-linkage", "-I", os.path.join(os.path.dirname(here), "include"),
                               "-I", os.path.join(os.path.dirname(here), "metric_depth_video_toolbox_amd", "csrc"), "-o", exe,
                               os.path.join(here, "ffv1_ycbcr_writer.cpp"),
                               os.path.join(os.path.dirname(here), "metric_depth_video_toolbox_amd", "csrc_host", "mdvt_ffv1_enc.cpp")])
    hs, vs = PIX_SHIFTS[pix_fmt]
    N, H, W = frames.shape[:3]
    if any((sx * W // slices[0]) % (1 << hs) for sx in range(slices[0])) or any((sy * H // slices[1]) % (1 << vs) for sy in range(slices[1])):
        raise SystemExit(f"{pix_fmt} in {slices[0]} x {slices[1]} slices of {W} x {H}: a slice origin is off the chroma grid -- no reader of "
                         "this project decodes such a stream (1080 rows in 8 slices start at multiples of 135)")
    y, cb, cr = ycbcr_planes(frames, hs, vs)
    raw, out = os.path.join(tmp, "planes.raw"), os.path.join(tmp, "packets.bin")
    with open(raw, "wb") as f:
        for t in range(N):
            f.write(y[t].tobytes() + cb[t].tobytes() + cr[t].tobytes())
    subprocess.check_call([exe, raw, str(W), str(H), str(N), str(hs), str(vs), str(slices[0]), str(slices[1]), "12", out])
    data = open(out, "rb").read()
    os.remove(raw)
    os.remove(out)
    n, = struct.unpack_from("<I", data, 0)
    cfg, o, packets = data[4:4 + n], 4 + n, []
    while o < len(data):
        n, = struct.unpack_from("<I", data, o)
        packets.append(data[o + 4:o + 4 + n])
        o += 4 + n
    assert len(packets) == N
    return packets, cfg


def decode_main(a):
    import tempfile
    import torch
    from metric_depth_video_toolbox_amd import _lib, clip, ffv1_device, video_io
    rng = np.random.default_rng(1)
    pool = ThreadPoolExecutor(a.host_threads)
    ctx = _lib.shared_context(0)
    stream = a.stream_class != "intra"
    rows = []
    nmax = max(int(v) for v in a.frames.split(","))
    tmp = tempfile.mkdtemp(prefix="ffv1_bench_")
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        pinned = torch.empty((nmax, H, W, 3), dtype=torch.uint8, pin_memory=True)
        d_host = torch.empty((nmax, H, W, 3), dtype=torch.uint8, device="cuda")
        d_dev = torch.empty((nmax, H, W, 3), dtype=torch.uint8, device="cuda")
        for kind in a.contents.split(","):
            frames = frames_of(kind, W, H, nmax, rng)
            for sl in a.slices.split(","):
                slices = tuple(int(v) for v in sl.split("x"))
                path = os.path.join(tmp, f"{size}_{kind}_{sl}.mkv")
                planar = a.pix_fmt != "rgb"
                if planar:
                    packets, cfg = ycbcr_stream(frames, a.pix_fmt, slices, tmp)
                elif stream:
                    with video_io.VideoWriter(path, W, H, 30.0, slices=slices, coder=0, gop=12, threads=a.host_threads) as w:
                        for f in frames:
                            w.write(f)
                    with video_io.VideoReader(path) as r:
                        cfg = r.config_record()
                        packets = [r.next_packet() for _ in range(len(frames))]
                else:
                    enc = list(pool.map(lambda f: video_io.encode_frame(f, slices=slices, threads=1), frames))
                    with video_io.VideoWriter(path, W, H, 30.0, slices=slices) as w:
                        for pkt, _ in enc:
                            w.write_packet(pkt)
                    packets, cfg = [e[0] for e in enc], enc[0][1]
                # an inter-coded file gets one reader (contexts carry over) with all the slice threads; an intra file the driver's two
                vf = None if planar else clip.VideoFrames(path, threads=a.host_threads) if stream else clip.VideoFrames(path)

                def host(n):                      # render_clip's load() + its H2D copy
                    h = pinned[:n].numpy()
                    if planar:                    # (no file: the host reader's decoder on the packets, all the slice threads)
                        with video_io.StreamDecoder(cfg, W, H, threads=a.host_threads) as d:
                            for t in range(n):
                                d.decode(packets[t], out=h[t])
                        d_host[:n].copy_(pinned[:n], non_blocking=True)
                        torch.cuda.synchronize()
                        return
                    half = 0 if stream else n // 2
                    jobs = [pool.submit(vf.read_into, h[:half], 0, half)] if half else []
                    jobs.append(pool.submit(vf.read_into, h[half:], half, n - half))
                    for j in jobs:
                        j.result()
                    d_host[:n].copy_(pinned[:n], non_blocking=True)
                    torch.cuda.synchronize()

                def device(staged):
                    enqueue = ffv1_device.enqueue_decode_stream if stream else ffv1_device.enqueue_decode
                    p = enqueue(ctx, staged, cfg, W, H, out=d_dev[:len(staged)])
                    p.done.synchronize()
                    flags = p.status.cpu()
                    if bool(flags.any()):
                        raise SystemExit(f"the device flagged {int((flags != 0).sum())} of {len(staged)} frames ({size}, {kind}, {sl}): "
                                         "not a device timing")
                for n in (int(v) for v in a.frames.split(",")):
                    staged = ffv1_device.StagedPackets(packets[:n])
                    host(n)
                    device(staged)
                    assert torch.equal(d_dev[:n], d_host[:n]) and (planar or np.array_equal(pinned[:n].numpy(), frames[:n])), (size, kind, sl, n)
                    dt_dev, dt_host = [], []
                    for _ in range(a.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        device(staged)
                        dt_dev.append(time.perf_counter() - t0)
                        t0 = time.perf_counter()
                        host(n)
                        dt_host.append(time.perf_counter() - t0)
                    r = dict(size=size, content=kind, slices=sl, frames=n, device_fps=n / min(dt_dev), host_fps=n / min(dt_host),
                             bytes_per_frame=staged.total / n)
                    r["speedup"] = r["device_fps"] / r["host_fps"]
                    if stream:
                        r["class"] = a.stream_class
                        r["pix_fmt"] = a.pix_fmt
                    rows.append(r)
                    print(f"decode {'' if not stream else a.stream_class + ' ' + a.pix_fmt + ' '}{size:>9} {kind:>9} {sl:>3} n={n:<3} device {r['device_fps']:8.1f} fps  host({a.host_threads}t) "
                          f"{r['host_fps']:8.1f} fps  x{r['speedup']:.2f}  {r['bytes_per_frame'] / 1e6:.2f} MB/frame", flush=True)
                if vf is not None:
                    vf.close()
                    os.remove(path)
    import shutil
    shutil.rmtree(tmp)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
