"""The device FFV1 stream decoder's host side -- no GPU: the decoder core (csrc/mdvt_ffv1_core.h: BitReader, Golomb-Rice, SliceDec)
compiled for the host, plain and with the sanitizers (tests/ffv1_stream_decode_host.cpp), on the stream matrix of
tests/ffv1_streams.py and on damaged packets; the class parser; the host entry points through ctypes; the device_all plumbing;
the opt-in writer class against oracle/ffv1_ref.py."""
import os
import re

import numpy as np
import pytest

import ffv1_streams as fs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vio():
    from metric_depth_video_toolbox_amd import video_io
    video_io.load()
    return video_io


@pytest.fixture(scope="module")
def ref():
    from oracle import ffv1_ref
    return ffv1_ref


@pytest.fixture(scope="module")
def programs():
    plain, why = fs.build_host_program(False)
    if plain is None:
        pytest.skip(why)
    asan, why = fs.build_host_program(True)                           # None only where the compiler has no sanitizer runtime
    if asan:
        fs.run_host_program(asan, [])                                  # an instrumented program that does not start is a failure
    return plain, asan, why


def _declared(header):
    hdr = open(os.path.join(REPO, "include", header)).read()
    return hdr, sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))


def test_the_entry_points_live_in_headers_of_their_own(vio):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    hdr, declared = _declared("mdvt_ffv1_stream_decode.h")
    assert declared == sorted(_lib.STREAM_DECODE_SYMBOLS)
    for s in _lib.STREAM_DECODE_SYMBOLS:
        assert hasattr(L, s) and s not in _lib.SYMBOLS and s not in _lib.DECODE_SYMBOLS
    for other in ("mdvt.h", "mdvt_ffv1_decode.h"):
        text = open(os.path.join(REPO, "include", other)).read()
        assert not any(s in text for s in _lib.STREAM_DECODE_SYMBOLS)
    assert L.mdvt_version() == 15
    nums = {k: int(v) for k, v in re.findall(r"#define (MDVT_FFV1_[A-Z_]+) (\d+)u", hdr)}
    assert nums == {"MDVT_FFV1_NO_KEY_FRAME": fs.NO_KEY_FRAME, "MDVT_FFV1_BROKEN_RUN": fs.BROKEN_RUN} and not set(nums.values()) & set(range(5))
    assert "not carried from one call to the next" in hdr
    _, declared = _declared("mdvt_video_stream.h")
    assert declared == sorted(vio.STREAM_SYMBOLS)
    for s in vio.STREAM_SYMBOLS:
        assert hasattr(vio.load(), s) and s not in vio.SYMBOLS


# ---------------------------------------------------------------------------------------------------------------------
# the core on the matrix
# ---------------------------------------------------------------------------------------------------------------------
def _check_matrix(exe):
    jobs, wants = [], []
    for case in fs.MATRIX:
        W, H, N = case[:3]
        frames, packets, cfg = fs.make_stream(case)
        for order, first_out in ((0, 0), (1, N // 2), (0, N - 1)):
            jobs.append((W, H, order, first_out, cfg, list(packets)))
            wants.append((case, order, first_out, frames))
    out = fs.run_host_program(exe, jobs)
    for (case, order, first_out, frames), res in zip(wants, out):
        assert res is not None, fs.case_id(case)
        assert res["status"] == [0] * case[2], (fs.case_id(case), res["status"])
        want = frames[first_out:, ..., ::-1] if order else frames[first_out:]
        assert np.array_equal(res["frames"], want), (fs.case_id(case), order, first_out)
    return dict(zip((fs.case_id(w[0]) for w in wants[::3]), out[::3]))


def test_the_matrix_streams_are_what_the_host_reader_reads():
    """The reference of every comparison here and on the GPU: the host reader returns the source frames, in both byte orders."""
    for case in fs.MATRIX:
        W, H, N = case[:3]
        frames, packets, cfg = fs.make_stream(case)
        for bgr in (False, True):
            got, err = fs.host_read(packets, cfg, W, H, bgr=bgr)
            assert err is None and len(got) == N
            assert np.array_equal(np.stack(got), frames[..., ::-1] if bgr else frames), fs.case_id(case)


def test_core_decodes_the_matrix_on_the_host(programs):
    plain, asan, why = programs
    by_case = _check_matrix(plain)                                     # (its byte accessors assert their bounds)
    # a stream that never enters the escape, the halving, a long run or a run cut by the row's end proves nothing
    c = by_case[fs.case_id(fs.COUNTERS_CASE)]
    print("counters", {k: c[k] for k in ("escapes", "halvings", "max_run_index", "short_tail_runs")})
    assert c["escapes"] > 0 and c["halvings"] > 0 and c["max_run_index"] >= 16 and c["short_tail_runs"] > 0
    assert max(r["max_run_index"] for r in by_case.values()) >= 20                   # 96x40, one slice: run lengths of 6 bits and more
    for case in fs.MATRIX:                                             # the range coder reads no Golomb-Rice code
        if case[3] == 1:
            r = by_case[fs.case_id(case)]
            assert (r["escapes"], r["halvings"], r["max_run_index"], r["short_tail_runs"]) == (0, 0, 0, 0)
    if asan is None:
        pytest.skip(f"no sanitizer build: {why}")
    _check_matrix(asan)


def test_a_call_that_starts_inside_a_run_and_a_flagged_frame(programs):
    """Frames in front of the call's first key frame: NO_KEY_FRAME, the rest decodes.  A CRC flip: CRC_MISMATCH on that frame,
    BROKEN_RUN up to the next key frame, the other runs intact."""
    plain, asan, why = programs
    case = fs.COUNTERS_CASE                                            # 7 frames, gop 3, ec 1: keys at 0, 3, 6
    W, H, N = case[:3]
    frames, packets, cfg = fs.make_stream(case)
    flipped = list(packets)
    b = bytearray(flipped[3]); b[len(b) // 2] ^= 0x10; flipped[3] = bytes(b)
    short = list(packets); short[4] = short[4][:2]
    for exe in (plain, asan):
        if exe is None:
            continue
        tail, crc, bad = fs.run_host_program(exe, [(W, H, 0, 0, cfg, list(packets[1:])), (W, H, 0, 0, cfg, flipped), (W, H, 0, 2, cfg, short)])
        assert tail["status"] == [fs.NO_KEY_FRAME] * 2 + [0] * 4 and np.array_equal(tail["frames"][2:], frames[3:])
        assert crc["status"] == [0, 0, 0, fs.CRC_MISMATCH, fs.BROKEN_RUN, fs.BROKEN_RUN, 0]
        assert np.array_equal(crc["frames"][:3], frames[:3]) and np.array_equal(crc["frames"][6], frames[6])
        assert bad["status"] == [0, 0, 0, 0, fs.BAD_PACKET, fs.BROKEN_RUN, 0]
        assert np.array_equal(bad["frames"][:2], frames[2:4]) and np.array_equal(bad["frames"][4], frames[6])


def test_the_intra_program_runs_the_same_decoder(tmp_path):
    """The two intra = 1 streams of the matrix (67x37, 2 frames, 3x2 slices, ec 1) through the intra decoder's host program
    (tests/ffv1_decode_host.cpp): the coder 1 stream packet by packet gives status 0 and the source frames, the coder 0 record is
    refused (verdict 100).  With test_core_decodes_the_matrix_on_the_host: both programs decode that stream with one SliceDec."""
    import test_video_decoder_cpu as intra
    range_case, golomb_case = (67, 37, 2, 1, 1, 1, 1, (3, 2)), (67, 37, 2, 0, 1, 1, 1, (3, 2))
    assert range_case in fs.MATRIX and golomb_case in fs.MATRIX
    W, H = range_case[:2]
    tmp = str(tmp_path)
    for sanitize in (False, True):
        exe, why = intra._build(tmp, sanitize)                         # (the plain build must succeed; the instrumented one may be missing,
        if exe is None or intra._run(exe, tmp, [])[0].returncode:      # or unable to start, as in test_video_decoder_cpu.py's fixture)
            assert sanitize, why
            continue
        frames, packets, cfg = fs.make_stream(range_case)
        r, out = intra._run(exe, tmp, [(W, H, 0, cfg, p) for p in packets])
        assert r.returncode == 0, r.stderr[-2000:]
        for (st, n, frame), want in zip(out, frames):
            assert st == 0 and n == 3 * W * H and np.array_equal(frame, want)
        _, packets, cfg = fs.make_stream(golomb_case)
        r, out = intra._run(exe, tmp, [(W, H, 0, cfg, packets[0])])
        assert r.returncode == 0 and out[0][0] == 100 and not out[0][2].any()


# ---------------------------------------------------------------------------------------------------------------------
# damaged packets: on the CPU, under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_core_survives_damaged_packets(programs, vio, ref):
    """Every run ends with a status and in-bounds accesses (asserting accessors, and the sanitizers where the compiler has them).
    A frame the core accepts is one the host accepts, with the host's bytes -- a truncated Golomb-Rice slice included, which the
    host decodes with zero bits; a frame the host refuses is flagged.  Where the host accepts and the core flags, the flag is
    BAD_SLICE_HEADER: slices that do not tile the frame, which the host decodes over each other (the one documented difference)."""
    plain, asan, why = programs
    for exe in (plain, asan):
        if exe is None:
            continue
        W, H, cfg, frame, res = fs.damaged_packets_verdicts(exe)
        assert len(res) > 1000
        assert res[0][1]["status"] == [0] and np.array_equal(res[0][1]["frames"][0], frame)
        accepted = differ = 0
        for v, r, host in res:
            st = r["status"][0]
            assert st in (0, 2, 3, 4, fs.NO_KEY_FRAME), st
            if host is None:
                assert st != 0, "the host refuses a frame the core accepts"
            elif st == 0:
                accepted += 1
                differ += not np.array_equal(host, frame)
                assert np.array_equal(r["frames"][0], host)
            else:
                assert st in (fs.BAD_SLICE_HEADER, fs.NO_KEY_FRAME), (st, len(v))     # the key-frame bit flipped: the host alone knows no run
        assert [(k, res[k][1]["status"][0]) for k, _ in fs.DAMAGED_PICKS] == list(fs.DAMAGED_PICKS)      # the GPU test's handful
        assert accepted >= 100 and differ >= 50                        # most damage to a Golomb-Rice payload still decodes: to other bytes
    if asan is None:
        pytest.skip(f"ran with asserting accessors only; no sanitizer build: {why}")


# ---------------------------------------------------------------------------------------------------------------------
# the class parser and the host entry points
# ---------------------------------------------------------------------------------------------------------------------
def _field(mode):
    if mode.get("version", 3) != 3:
        return "version"
    if mode.get("coder") == 2:
        return "coder_type 2"
    if mode.get("alpha"):
        return "extra_plane"
    if mode.get("five"):
        return "quantisation tables"
    return None


def test_class_parser_on_every_mode_the_host_reader_claims(vio, ref, tmp_path):
    import test_video_cpu
    from metric_depth_video_toolbox_amd import _lib, ffv1_device as fd
    L = _lib.load()
    seen = set()
    for mode in test_video_cpu.MODES:
        m = dict(mode)
        gop, custom = m.pop("gop"), m.pop("custom", False)
        if custom:
            one = list(ref.DEFAULT_ONE)
            for i in range(20, 200, 7):
                one[i] = min(248, one[i] + 3)
            m["custom"] = one
        p = ref.Params(**m)
        W, H = 16, 8
        enc = ref.StreamEncoder(p, W, H, gop=gop)
        packets = [enc.encode(np.zeros((H, W, 4 if p.alpha else 3), np.uint8)) for _ in range(2)]
        path = str(tmp_path / "m.mkv")
        with open(path, "wb") as f:
            f.write(ref.mux_matroska(packets, W, H, 30, ref.config_record(p) if p.version >= 2 else b""))
        with vio.VideoReader(path) as r:
            cfg = r.config_record()
            why, why_info = fd.stream_supported(r.info, cfg), fd.stream_supported(r.info)
        field = _field(mode)
        seen.add(field)
        if field is None:
            assert why is None and why_info is None, (mode, why)
            assert L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg)) is None
        else:
            assert why is not None and field in why, (mode, why)
            if p.version == 3:
                raw = L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg))
                assert raw is not None and field in raw.decode(), (mode, raw)
            if field != "quantisation tables":
                assert why_info is not None and field in why_info
    assert seen == {None, "version", "coder_type 2", "extra_plane", "quantisation tables"}
    assert b"configuration record" in L.mdvt_ffv1_stream_decode_supported(b"", 0)
    # the old parser is where it was: it still refuses what only the new one takes
    cfg = ref.config_record(ref.Params(coder=0, intra=0))
    assert b"coder_type" in L.mdvt_ffv1_decode_supported(cfg, len(cfg)) and L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg)) is None
    cfg = ref.config_record(ref.Params(intra=0))
    assert b"intra" in L.mdvt_ffv1_decode_supported(cfg, len(cfg)) and L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg)) is None


def test_packet_is_key_through_ctypes(ref):
    from metric_depth_video_toolbox_amd import _lib, ffv1_device as fd
    L = _lib.load()
    for case in fs.MATRIX:
        _, packets, _ = fs.make_stream(case)
        assert [L.mdvt_ffv1_packet_is_key(p, len(p)) for p in packets] == [int(k) for k in fs.key_flags(case)], fs.case_id(case)
        assert [fd.packet_is_key(p) for p in packets] == fs.key_flags(case)
    assert L.mdvt_ffv1_packet_is_key(b"\xff\xff", 2) == -1 and L.mdvt_ffv1_packet_is_key(None, 0) == -1
    assert L.mdvt_ffv1_packet_is_key(b"\xff\xff\x00", 3) == 1 and L.mdvt_ffv1_packet_is_key(b"\x00\x00\x00", 3) == 0
    assert L.mdvt_ffv1_packet_is_key(b"\x7f\x80\x00", 3) == 1 and L.mdvt_ffv1_packet_is_key(b"\x7f\x7f\x00", 3) == 0     # the bound of state 128


# ---------------------------------------------------------------------------------------------------------------------
# device_all: the flag and the key-frame back-scan (no device)
# ---------------------------------------------------------------------------------------------------------------------
def test_device_all_is_a_decoder_everywhere_device_is():
    from metric_depth_video_toolbox_amd import (basic_nomal_infill as bni, clip, clip_io, find_convergence_depth as fcd,
                                                stereo_crafter_infill as sci, stereo_rerender as sr, video_metric_convert as vmc)
    assert clip_io.VIDEO_DECODERS == ("host", "device", "device_all") and clip_io.KEY_SCAN_FRAMES >= 24
    assert clip.check_video_decoder("device_all", True) == "device_all"
    with pytest.raises(ValueError, match="video_decoder device_all"):
        clip.check_video_decoder("device_all", False)                  # .npy inputs
    with pytest.raises(ValueError, match="video_decoder device decodes"):
        clip.check_video_decoder("device", False)
    a = sr.build_arg_parser().parse_args(["--depth_video", "d.mkv", "--xfov", "45", "--video_decoder", "device_all"])
    assert a.video_decoder == "device_all"
    for mod in (bni, fcd, sci, vmc):
        act = [x for x in mod.build_parser()._actions if "--video_decoder" in x.option_strings][0]
        assert tuple(act.choices) == clip_io.VIDEO_DECODERS and act.default == "host", mod.__name__


def test_key_frame_back_scan_on_a_file(vio, ref, tmp_path, capfd, monkeypatch):
    from metric_depth_video_toolbox_amd import clip_io
    W, H, N, gop = 8, 6, 30, 25
    frames = fs.stream_content(N, H, W, 2)
    path = str(tmp_path / "s.mkv")
    with vio.VideoWriter(path, W, H, 30, slices=(2, 1), coder=0, gop=gop) as w:
        for f in frames:
            w.write(f)
    v = clip_io.VideoFrames(path)
    assert v.use_device_decoder("depth video", "device_all") and v.device_decode and v.stream_decode
    with vio.VideoReader(path) as r:
        packets = [r.next_packet() for _ in range(N)]
    for a, n in ((0, 3), (1, 2), (24, 3), (25, 5), (27, 3), (29, 1)):
        got, first_out = v.read_stream_packets(a, n)
        key = a // gop * gop
        assert first_out == a - key and got == packets[key:a + n], (a, n)       # 24 frames back included
    assert capfd.readouterr().err == ""
    # a key frame further back than the bound: None, and the file goes to the host with one line
    monkeypatch.setattr(clip_io, "KEY_SCAN_FRAMES", 5)
    assert v.read_stream_packets(3, 2) is not None and v.read_stream_packets(24, 2) is None
    v.host_after_far_key_frame()
    v.host_after_far_key_frame()
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "decoded on the host" in err and "intra" in err and "key-frame distance" in err and "depth video" in err
    assert not v.device_decode
    assert np.array_equal(np.asarray(v[22:26]), frames[22:26])         # and reads on there
    v.close()
    # "device" keeps handing such a file to the host, with the line it always printed; an old-class file takes the old call
    v = clip_io.VideoFrames(path)
    assert not v.use_device_decoder("depth video") and not v.stream_decode
    assert "video_decoder device: depth video" in capfd.readouterr().err
    v.close()
    old = str(tmp_path / "o.mkv")
    with vio.VideoWriter(old, W, H, 30) as w:
        w.write(frames[0])
    v = clip_io.VideoFrames(old)
    assert v.use_device_decoder("color video", "device_all") and v.device_decode and not v.stream_decode
    v.close()


# ---------------------------------------------------------------------------------------------------------------------
# the writer of the class
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,N,gop,slices", [(67, 37, 7, 3, (3, 2)), (96, 40, 6, 5, (1, 1)), (5, 4, 5, 2, (4, 2)), (67, 37, 3, 99, (1, 37)),
                                              (67, 37, 2, 1, (67, 1)), (2, 2, 4, 3, (2, 2)), (1, 1, 4, 2, (1, 1))])
def test_the_stream_writer_is_byte_identical_to_the_oracle(vio, ref, tmp_path, W, H, N, gop, slices):
    frames = fs.stream_content(N, H, W, 9)
    p = ref.Params(coder=0, intra=0, nh=slices[0], nv=slices[1])
    enc = ref.StreamEncoder(p, W, H, gop=gop)
    want = [enc.encode(f) for f in frames]
    path = str(tmp_path / "w.mkv")
    with vio.VideoWriter(path, W, H, 30, slices=slices, coder=0, gop=gop, bgr=True, threads=3) as w:
        for f in frames:
            w.write(np.ascontiguousarray(f[..., ::-1]))
    with vio.VideoReader(path) as r:
        assert (r.info.coder_type, r.info.intra, r.info.ec, r.info.slices, r.frames) == (0, 0, 1, slices[0] * slices[1], N)
        assert r.config_record() == ref.config_record(p)
        assert [r.next_packet() for _ in range(N)] == want
    with vio.VideoReader(path) as r:
        assert np.array_equal(np.stack(list(r)), frames)
    with vio.StreamDecoder(ref.config_record(p), W, H, bgr=True) as d:             # the packets alone, state carried along
        assert all(np.array_equal(d.decode(pk), f[..., ::-1]) for pk, f in zip(want, frames))
    with pytest.raises(vio.VideoError):
        with vio.StreamDecoder(ref.config_record(p), W, H) as d:
            d.decode(want[1] if gop > 1 else b"\x00\x00\x00\x00")


def test_the_default_writer_is_unchanged(vio, tmp_path):
    """coder=1 (the default) writes what it wrote: the old class, every block a key frame."""
    frames = fs.stream_content(3, 9, 12, 1)
    path = str(tmp_path / "d.mkv")
    with vio.VideoWriter(path, 12, 9, 30, slices=(2, 2)) as w:
        for f in frames:
            w.write(f)
    with vio.VideoReader(path) as r:
        assert (r.info.coder_type, r.info.intra) == (1, 1)
        assert [r.next_packet() for _ in range(3)] == [vio.encode_frame(f, slices=(2, 2))[0] for f in frames]
    with pytest.raises(ValueError, match="coder"):
        vio.VideoWriter(str(tmp_path / "x.mkv"), 12, 9, 30, coder=2)
