"""The device FFV1 decoder's host side -- no GPU: the new entry point's binding, ffv1_device.supported() on every mode the
independent encoder writes, the slice-table walk against the host reader's own acceptance, and the decoder core
(csrc/mdvt_ffv1_core.h) compiled for the host with the sanitizers (tests/ffv1_decode_host.cpp) on good and on corrupted packets."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")


@pytest.fixture(scope="module")
def vio():
    from metric_depth_video_toolbox_amd import video_io
    video_io.load()
    return video_io


@pytest.fixture(scope="module")
def ref():
    from oracle import ffv1_ref
    return ffv1_ref


def test_the_entry_point_is_exported_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "mdvt_ffv1_decode.h")).read()
    declared = sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert declared == sorted(_lib.DECODE_SYMBOLS)
    for s in _lib.DECODE_SYMBOLS:
        assert hasattr(L, s) and s not in _lib.SYMBOLS
    main = open(os.path.join(REPO, "include", "mdvt.h")).read()
    assert "mdvt_decode_video_frames" not in main
    assert L.mdvt_version() == 15                                   # ABI 0.15: include/mdvt.h is unchanged
    for doc in ("sr:326-341", "489-509", "bni:129-171"):
        assert doc.split(":")[-1] in hdr


def _custom_table(ref):
    one = list(ref.DEFAULT_ONE)
    for i in range(20, 200, 7):
        one[i] = min(248, one[i] + 3)
    return one


MODES = [(dict(), None), (dict(ec=0), None), (dict(nh=4, nv=4), None), (dict(nh=16, nv=64), None), (dict(micro=3, nh=2), None),
         (dict(coder=0), "coder_type"), (dict(coder=0, intra=0), "coder_type"), (dict(intra=0), "intra"), (dict(version=1), "version"),
         (dict(version=1, coder=0), "version"), (dict(version=0, coder=0), "version"), (dict(alpha=1), "extra_plane"),
         (dict(coder=2, custom=True), "coder_type"), (dict(five=True), "quantisation tables"), (dict(five=True, coder=0), "coder_type")]


@pytest.mark.parametrize("kw,field", MODES, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_supported_names_the_field(vio, ref, tmp_path, kw, field):
    from metric_depth_video_toolbox_amd import ffv1_device as fd
    kw = dict(kw)
    if kw.pop("custom", False):
        kw["custom"] = _custom_table(ref)
    p = ref.Params(**kw)
    W, H = 64, 64
    rng = np.random.default_rng(3)
    enc = ref.StreamEncoder(p, W, H, gop=1 if p.intra else 2)
    packets = [enc.encode(rng.integers(0, 256, (H, W, 4 if p.alpha else 3), dtype=np.uint8) // 64 * 64) for _ in range(2)]
    path = str(tmp_path / "m.mkv")
    with open(path, "wb") as f:
        f.write(ref.mux_matroska(packets, W, H, 30, ref.config_record(p) if p.version >= 2 else b""))
    with vio.VideoReader(path) as r:
        why = fd.supported(r.info, r.config_record())
        why_info = fd.supported(r.info)
    if field is None:
        assert why is None and why_info is None
    else:
        assert why is not None and field in why, why
        if field != "quantisation tables":                         # (the tables are not part of VideoInfo: the record decides)
            assert why_info is not None and field in why_info


def test_flags_and_value_errors():
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, clip, stereo_rerender as sr
    for value in ("host", "device"):
        assert clip.check_video_decoder(value, True) == value
    assert clip.check_video_decoder("host", False) == "host"
    with pytest.raises(ValueError, match="video_decoder"):
        clip.check_video_decoder("device", False)                   # .npy inputs
    with pytest.raises(ValueError, match="video_decoder"):
        clip.check_video_decoder("gpu", True)
    a = sr.build_arg_parser().parse_args(["--depth_video", "d.mkv", "--color_video", "c.mkv", "--xfov", "45"])
    assert a.video_decoder == "host" and a.video_encoder == "host"
    a = sr.build_arg_parser().parse_args(["--depth_video", "d.mkv", "--color_video", "c.mkv", "--xfov", "45", "--video_decoder", "device"])
    assert a.video_decoder == "device"
    b = bni.build_parser().parse_args(["--sbs_color_video", "a.mkv", "--sbs_mask_video", "b.mkv"])
    assert (b.video_decoder, b.video_encoder, b.batch) == ("host", "host", 8)
    b = bni.build_parser().parse_args(["--sbs_color_video", "a.mkv", "--sbs_mask_video", "b.mkv", "--video_decoder", "device",
                                       "--video_encoder", "device", "--batch", "16"])
    assert (b.video_decoder, b.video_encoder, b.batch) == ("device", "device", 16)


# ---------------------------------------------------------------------------------------------------------------------
# the decoder core on the host
# ---------------------------------------------------------------------------------------------------------------------
def _build(tmp, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = os.path.join(tmp, "ffv1_decode_host_asan" if sanitize else "ffv1_decode_host")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, os.path.join(REPO, "tests", "ffv1_decode_host.cpp")]
    if sanitize:
        cmd[3:3] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and sanitize:
        return None, r.stderr[-400:]
    assert r.returncode == 0, r.stderr[-2000:]
    return exe, ""


def _run(exe, tmp, jobs, timeout=600):
    """jobs: (W, H, order, config, packet) -> [(status, samples, frame)]"""
    jp, rp = os.path.join(tmp, "jobs.bin"), os.path.join(tmp, "results.bin")
    with open(jp, "wb") as f:
        f.write(struct.pack("<I", len(jobs)))
        for W, H, order, cfg, pkt in jobs:
            f.write(struct.pack("<5I", W, H, order, len(cfg), len(pkt)) + cfg + pkt)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:verify_asan_link_order=0")
    r = subprocess.run([exe, jp, rp], capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode:
        return r, None
    data, o, out = open(rp, "rb").read(), 0, []
    for W, H, *_ in jobs:
        st, n = struct.unpack_from("<2I", data, o)
        out.append((st, n, np.frombuffer(data, np.uint8, W * H * 3, o + 8).reshape(H, W, 3)))
        o += 8 + W * H * 3
    assert o == len(data)
    return r, out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ffv1_core"))
    plain, _ = _build(tmp, False)
    asan, why = _build(tmp, True)
    if asan:                                                           # can the instrumented program start here at all?
        r, out = _run(asan, tmp, [])
        if r.returncode:
            asan, why = None, f"the instrumented program does not start: {r.stderr[-300:]}"
    return tmp, plain, asan, why


def _good_jobs(vio, ref):
    rng = np.random.default_rng(1)
    jobs, want = [], []
    for W, H, sl in [(1, 1, (1, 1)), (2, 2, (2, 2)), (17, 9, (3, 5)), (17, 9, (17, 9)), (64, 48, (4, 4)), (250, 61, (8, 8)), (250, 61, (16, 61))]:
        for kind in range(3):
            f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == 0 else np.full((H, W, 3), (0, 255, 77)[kind], np.uint8)
            pkt, cfg = vio.encode_frame(f, slices=sl)
            jobs.append((W, H, kind % 2, cfg, pkt))
            want.append(f[..., ::-1] if kind % 2 else f)
        if W <= 64:
            f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            p = ref.Params(nh=sl[0], nv=sl[1], ec=0)
            jobs.append((W, H, 0, ref.config_record(p), ref.StreamEncoder(p, W, H).encode(f)))
            want.append(f)
    return jobs, want


def _check_good(exe, tmp, vio, ref):
    jobs, want = _good_jobs(vio, ref)
    r, out = _run(exe, tmp, jobs)
    assert r.returncode == 0, r.stderr[-2000:]
    for (W, H, order, cfg, pkt), (st, n, frame), f in zip(jobs, out, want):
        assert st == 0 and n == 3 * W * H and np.array_equal(frame, f), (W, H, st)
        assert np.array_equal(vio.decode_frame(pkt, cfg, W, H, bgr=bool(order)), f)


def test_core_decodes_in_class_packets_on_the_host(programs, vio, ref):
    tmp, plain, asan, why = programs
    _check_good(plain, tmp, vio, ref)                                  # (its byte accessors assert their bounds)
    if asan is None:
        pytest.skip(f"no sanitizer build: {why}")
    _check_good(asan, tmp, vio, ref)


def _corruptions(ref, n_each=110):
    """Seeded corruptions of three small packets without CRCs: whatever is in them reaches the range decoder."""
    rng = np.random.default_rng(20261016)
    jobs = []
    for W, H, nh, nv in ((24, 16, 2, 2), (40, 9, 3, 1), (9, 30, 1, 4)):
        p = ref.Params(nh=nh, nv=nv, ec=0)
        cfg = ref.config_record(p)
        pkt = ref.StreamEncoder(p, W, H).encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        for k in range(n_each):
            b = bytearray(pkt)
            kind = k % 4
            if kind == 0:
                for _ in range(1 + k % 5):
                    b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:
                b = b[:int(rng.integers(0, len(b)))]
            elif kind == 2:
                cut = int(rng.integers(0, len(b)))
                b = b[:cut] + bytearray(rng.integers(0, 256, len(pkt) - cut, dtype=np.uint8).tobytes())
            else:                                                      # the payload damaged, the slice sizes intact
                i = int(rng.integers(0, max(1, len(b) - 3 * nh * nv)))
                b[i:i + 4] = rng.integers(0, 256, len(b[i:i + 4]), dtype=np.uint8).tobytes()
            jobs.append((W, H, 0, cfg, bytes(b)))
    return jobs


def test_core_survives_corrupted_packets(programs, vio, ref):
    """Every run ends within the sample-count bound with a status or a frame; the bounds hold (asserting accessors, and the
    sanitizers where the compiler has them); the frames the host reader accepts decode to the host's bytes with status 0, and a
    frame the host refuses is flagged."""
    tmp, plain, asan, why = programs
    jobs = _corruptions(ref)
    assert len(jobs) >= 300
    for exe in (plain, asan):
        if exe is None:
            continue
        r, out = _run(exe, tmp, jobs)
        assert r.returncode == 0, r.stderr[-2000:]
        accepted = 0
        for (W, H, _, cfg, pkt), (st, n, frame) in zip(jobs, out):
            assert st in (0, 2, 3, 4) and n <= 3 * W * H
            try:
                host = vio.decode_frame(pkt, cfg, W, H)
            except vio.VideoError:
                host = None
            if host is None:
                assert st != 0, "the host refuses a frame the core accepts"
            elif st == 0:
                accepted += 1
                assert np.array_equal(frame, host)
        assert accepted >= 3                                           # (some corruptions leave a decodable stream)
    if asan is None:
        pytest.skip(f"ran with asserting accessors only; no sanitizer build: {why}")


def test_slice_walk_matches_the_host_readers_acceptance(programs, vio, ref):
    """Packets with CRCs, damaged where the walk or the CRC must catch it: status != 0 exactly where the host refuses."""
    tmp, plain, asan, why = programs
    rng = np.random.default_rng(77)
    W, H = 40, 22
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pkt, cfg = vio.encode_frame(f, slices=(3, 2))
    variants = [pkt, pkt[:-1], pkt[:-9], pkt[:2], b"", b"\x00" * 7 + pkt, pkt + b"\x00", pkt[: len(pkt) // 2]]
    b = bytearray(pkt); b[-8:-5] = b"\xff\xff\xff"; variants.append(bytes(b))
    b = bytearray(pkt); b[-8:-5] = b"\x00\x00\x00"; variants.append(bytes(b))
    for k in range(40):
        b = bytearray(pkt)
        b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        variants.append(bytes(b))
    r, out = _run(plain, tmp, [(W, H, 0, cfg, v) for v in variants])
    assert r.returncode == 0, r.stderr[-2000:]
    for v, (st, n, frame) in zip(variants, out):
        try:
            host = vio.decode_frame(v, cfg, W, H)
        except vio.VideoError:
            host = None
        assert (st == 0) == (host is not None), (len(v), st)
        if host is not None:
            assert np.array_equal(frame, host)
    assert out[0][0] == 0 and sum(1 for o in out if o[0] == 0) <= 2
