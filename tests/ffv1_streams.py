"""Shared by the stream decoder's tests (CPU and GPU): the fixture content, the streams oracle/ffv1_ref.py makes of it, the host
reader's frames for them, and the host program of tests/ffv1_stream_decode_host.cpp.  Everything is made once per process."""
import functools
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")

NO_KEY_FRAME, BROKEN_RUN = 5, 6
CRC_MISMATCH, BAD_SLICE_HEADER, DAMAGED, BAD_PACKET = 1, 2, 3, 4


def stream_content(N, H, W, seed):
    """Frame t: flat 40 + 3t; the middle third holds ramps; right of the middle every third band of four rows holds noise; the
    last two rows are flat 200.  Flat runs of every length, runs cut by the row's end, escapes and state halvings."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((N, H, W, 3), np.uint8)
    for t in range(N):
        f = np.full((H, W, 3), (40 + 3 * t) % 256, np.uint8)
        mid = (x >= W // 3) & (x < W - W // 3)
        for c, m in enumerate((3, 5, 7)):
            f[..., c][mid] = (((x + y + t) * m) % 256)[mid]
        noisy = (x > W // 2) & ((y // 4 + t) % 3 == 0)
        f[noisy] = rng.integers(0, 256, (int(noisy.sum()), 3), dtype=np.uint8)
        f[max(0, H - 2):] = 200
        out[t] = f
    return out


# (W, H, frames, coder, ec, gop, intra, (nh, nv)): coder 0 / 1, ec 0 / 1, gop 1, 2, 3, 5 and past the end, intra = 1, the slice
# grids (1,1), (3,2), (4,2), (67,1), (1,37), the sizes 1x1, 2x2, 5x4, 67x37, 96x40
MATRIX = [
    (67, 37, 7, 0, 1, 3, 0, (3, 2)),           # the case whose counters are asserted
    (67, 37, 7, 1, 0, 3, 0, (3, 2)),
    (67, 37, 3, 0, 0, 1, 0, (67, 1)),
    (67, 37, 3, 0, 1, 99, 0, (1, 37)),
    (67, 37, 3, 1, 1, 2, 0, (1, 37)),
    (67, 37, 2, 0, 1, 1, 1, (3, 2)),
    (67, 37, 2, 1, 1, 1, 1, (3, 2)),
    (96, 40, 6, 0, 0, 5, 0, (1, 1)),
    (96, 40, 3, 1, 1, 2, 0, (4, 2)),
    (5, 4, 5, 0, 1, 2, 0, (4, 2)),
    (5, 4, 5, 1, 0, 5, 0, (4, 2)),
    (2, 2, 4, 0, 0, 3, 0, (1, 1)),
    (2, 2, 4, 1, 1, 2, 0, (2, 2)),
    (1, 1, 4, 0, 1, 2, 0, (1, 1)),
    (1, 1, 4, 1, 0, 99, 0, (1, 1)),
]
COUNTERS_CASE = MATRIX[0]


def case_id(c):
    W, H, N, coder, ec, gop, intra, (nh, nv) = c
    return f"{W}x{H}x{N}-coder{coder}-ec{ec}-gop{gop}-intra{intra}-{nh}x{nv}"


@functools.lru_cache(maxsize=None)
def make_stream(case, seed=11):
    """-> (frames N x H x W x 3 RGB, packets, configuration record)"""
    from oracle import ffv1_ref as ref
    W, H, N, coder, ec, gop, intra, (nh, nv) = case
    frames = stream_content(N, H, W, seed)
    p = ref.Params(coder=coder, ec=ec, intra=intra, nh=nh, nv=nv)
    enc = ref.StreamEncoder(p, W, H, gop=gop)
    return frames, tuple(enc.encode(f) for f in frames), ref.config_record(p)


def host_read(packets, config, W, H, bgr=False):
    """The host reader on the packets in order, through a Matroska file -> (frames read, error text or None)."""
    from metric_depth_video_toolbox_amd import video_io
    from oracle import ffv1_ref as ref
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s.mkv")
        with open(path, "wb") as f:
            f.write(ref.mux_matroska(list(packets), W, H, 30, config))
        out = []
        with video_io.VideoReader(path, bgr=bgr, threads=1) as r:
            try:
                for fr in r:
                    out.append(fr)
            except video_io.VideoError as e:
                return out, str(e)
    return out, None


def key_flags(case):
    W, H, N, coder, ec, gop, intra, sl = case
    return [t % gop == 0 for t in range(N)]


# ------------------------------------------------------------------------------------------------------- the host program
_programs = {}


def build_host_program(sanitize):
    """-> (path, None) or (None, why)"""
    if sanitize in _programs:
        return _programs[sanitize]
    gxx = shutil.which("g++")
    if not gxx:
        _programs[sanitize] = (None, "no g++")
        return _programs[sanitize]
    tmp = tempfile.mkdtemp(prefix="ffv1_stream_core_")
    exe = os.path.join(tmp, "ffv1_stream_decode_host_asan" if sanitize else "ffv1_stream_decode_host")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, os.path.join(REPO, "tests", "ffv1_stream_decode_host.cpp")]
    if sanitize:
        cmd[3:3] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    # the one reason to go without the instrumented program: this compiler has no sanitizer runtime to link.  Anything else that
    # breaks the instrumented build (a warning that only fires under its flags, say) is a failure.
    no_runtime = any(t in r.stderr for t in ("cannot find -lasan", "cannot find -lubsan", "libasan.a", "libubsan.a", "unrecognized"))
    if r.returncode and sanitize and no_runtime:
        _programs[sanitize] = (None, r.stderr[-400:])
    else:
        assert r.returncode == 0, r.stderr[-3000:]
        _programs[sanitize] = (exe, None)
    return _programs[sanitize]


def run_host_program(exe, jobs, timeout=900):
    """jobs: (W, H, order, first_out, config, packets) -> [None (record refused) or dict(status, frames, escapes, halvings,
    max_run_index, short_tail_runs)]; raises AssertionError with the program's stderr when it does not end cleanly."""
    with tempfile.TemporaryDirectory() as tmp:
        jp, rp = os.path.join(tmp, "jobs.bin"), os.path.join(tmp, "results.bin")
        with open(jp, "wb") as f:
            f.write(struct.pack("<I", len(jobs)))
            for W, H, order, first_out, cfg, packets in jobs:
                f.write(struct.pack("<6I", W, H, order, first_out, len(cfg), len(packets)) + cfg)
                for p in packets:
                    f.write(struct.pack("<I", len(p)) + p)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
        r = subprocess.run([exe, jp, rp], capture_output=True, text=True, timeout=timeout, env=env)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        data, o, out = open(rp, "rb").read(), 0, []
    for W, H, order, first_out, cfg, packets in jobs:
        verdict, esc, halv, mri, tails = struct.unpack_from("<5I", data, o)
        o += 20
        if verdict:
            out.append(None)
            continue
        n = len(packets)
        status = list(struct.unpack_from(f"<{n}I", data, o))
        o += 4 * n
        frames = np.frombuffer(data, np.uint8, (n - first_out) * H * W * 3, o).reshape(n - first_out, H, W, 3)
        o += frames.size
        out.append(dict(status=status, frames=frames, escapes=esc, halvings=halv, max_run_index=mri, short_tail_runs=tails))
    assert o == len(data)
    return out


# ------------------------------------------------------------------------------------------------------- damaged packets
def _damage_jobs():
    """One small Golomb-Rice key frame without CRCs, so that whatever is in it reaches the decoder: every single-bit flip, every
    truncation, and seeded random corruptions."""
    from oracle import ffv1_ref as ref
    W, H, nh, nv = 13, 9, 2, 2
    frames = stream_content(1, H, W, 5)
    p = ref.Params(coder=0, ec=0, intra=0, nh=nh, nv=nv)
    cfg, pkt = ref.config_record(p), ref.StreamEncoder(p, W, H, gop=4).encode(frames[0])
    variants = [pkt]
    for i in range(len(pkt) * 8):
        b = bytearray(pkt); b[i >> 3] ^= 0x80 >> (i & 7); variants.append(bytes(b))
    variants += [pkt[:k] for k in range(len(pkt))]
    rng = np.random.default_rng(20261019)
    for k in range(300):
        b = bytearray(pkt)
        if k % 3 == 0:
            for _ in range(2 + k % 5):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif k % 3 == 1:
            cut = int(rng.integers(0, len(b)))
            b = b[:cut] + bytearray(rng.integers(0, 256, len(pkt) - cut, dtype=np.uint8).tobytes())
        else:                                                          # the payload damaged, the slice sizes intact
            i = int(rng.integers(0, max(1, len(b) - 3 * nh * nv)))
            b[i:i + 4] = rng.integers(0, 256, len(b[i:i + 4]), dtype=np.uint8).tobytes()
        variants.append(bytes(b))
    return W, H, cfg, pkt, frames[0], variants


# (index into _damage_jobs()'s variants, the core's status word): a fixed handful for the GPU, which needs no compiler for them;
# tests/test_video_stream_decoder_cpu.py asserts that the host program gives exactly these
DAMAGED_PICKS = ((0, 0), (17, 0), (140, 0), (333, 0), (700, 0), (2644, 0), (2793, 0), (1, NO_KEY_FRAME), (2454, NO_KEY_FRAME),
                 (2495, NO_KEY_FRAME), (2, BAD_SLICE_HEADER), (5, BAD_SLICE_HEADER), (265, BAD_SLICE_HEADER))


def damaged_picks():
    """-> W, H, configuration record, [(packet, expected status)] of DAMAGED_PICKS"""
    W, H, cfg, pkt, frame, variants = _damage_jobs()
    return W, H, cfg, [(variants[k], st) for k, st in DAMAGED_PICKS]


def damaged_packets_verdicts(exe):
    """[(variant, core status, host frame or None)] -- shared with the GPU test, which takes a handful of these."""
    from metric_depth_video_toolbox_amd import video_io as vio
    W, H, cfg, pkt, frame, variants = _damage_jobs()
    out = run_host_program(exe, [(W, H, 0, 0, cfg, [v]) for v in variants])
    res = []
    for v, r in zip(variants, out):
        try:
            host = vio.decode_frame(v, cfg, W, H)
        except vio.VideoError:
            host = None
        res.append((v, r, host))
    return W, H, cfg, frame, res
