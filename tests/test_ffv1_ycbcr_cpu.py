"""YCbCr FFV1 (yuv444p, yuv422p, yuv420p) on the host -- no GPU: the reference coder of tests/ffv1_ycbcr_ref.py round-trips; the
host reader (libmdvt_video.so) and the packet-to-packet decoder return exactly convert(planes) for the matrix; the conversion's
known answers; the refusals with their messages; pix_fmt; and the device decoder's core with its planar mode compiled for the
host, plain and under the sanitizers (tests/ffv1_ycbcr_decode_host.cpp, a program of its own), on the matrix and on damaged packets.
The planes are exact by RFC 9043; the conversion is this project's decree (include/mdvt_video.h), not a claim about cv2's bits."""
import glob
import os

import numpy as np
import pytest

import ffv1_streams as fs
import ffv1_ycbcr_ref as yr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vio():
    from metric_depth_video_toolbox_amd import video_io
    video_io.load()
    return video_io


@pytest.fixture(scope="module")
def programs():
    plain, why = yr.build_host_program(False)
    if plain is None:
        pytest.skip(why)
    asan, why = yr.build_host_program(True)                           # None only where the compiler has no sanitizer runtime
    if asan:
        fs.run_host_program(asan, [])                                  # an instrumented program that does not start is a failure
    return plain, asan, why


# ---------------------------------------------------------------------------------------------------------------------
# the reference coder and the conversion
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix", list(yr.PIX_FMTS))
@pytest.mark.parametrize("coder", (0, 1))
def test_reference_round_trip(pix, coder):
    """Random planes (escapes, every context) and flat planes (runs that span rows) through the reference encoder and decoder, inter
    frames included, in one slice at an odd size and in 2 x 2 slices."""
    hs, vs = yr.PIX_FMTS[pix]
    rng = np.random.default_rng(7 + coder)
    for W, H, sl in ((13, 9, (1, 1)), (20, 12, (2, 2))):
        ch, cw = yr.chroma_shape(W, H, hs, vs)
        assert (ch, cw) == (-(-H // (1 << vs)), -(-W // (1 << hs)))
        frames = [tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (ch, cw), (ch, cw))),
                  (np.full((H, W), 77, np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 3, np.uint8)),
                  (np.full((H, W), 77, np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 3, np.uint8))]
        frames.append(tuple(rng.integers(100, 104, s, dtype=np.uint8) for s in ((H, W), (ch, cw), (ch, cw))))
        p = yr.Params(pix_fmt=pix, coder=coder, intra=0, nh=sl[0], nv=sl[1])
        enc, dec = yr.Encoder(p, W, H, gop=3), yr.Decoder(p, W, H)
        sizes = []
        for planes in frames:
            pkt = enc.encode(planes)
            sizes.append(len(pkt))
            got = dec.decode(pkt)
            assert all(np.array_equal(a, b) for a, b in zip(got, planes))
        assert sizes[1] < sizes[0] // 4 and sizes[2] <= sizes[1]       # a flat frame is runs


def test_conversion_known_answers():
    """Computed by hand from the formula of include/mdvt_video.h."""
    known = {(16, 128, 128): (0, 0, 0), (235, 128, 128): (255, 255, 255), (0, 0, 0): (0, 135, 0), (255, 255, 255): (255, 125, 255),
             (81, 90, 240): (255, 0, 0), (145, 54, 34): (0, 255, 1)}
    # (0, 0, 0):       c -16 d -128 e -128: R (-4768 - 52352 + 128) >> 8 < 0; G (-4768 + 12800 + 26624 + 128) >> 8 = 34784 >> 8 = 135; B < 0
    # (255, 255, 255): c 239 d 127 e 127:   R (71222 + 51943 + 128) >> 8 = 481 -> 255; G (71222 - 12700 - 26416 + 128) >> 8 = 32234 >> 8 = 125; B -> 255
    # (81, 90, 240):   c 65 d -38 e 112:    R (19370 + 45808 + 128) >> 8 = 255; G (19370 + 3800 - 23296 + 128) >> 8 = 2 >> 8 = 0; B (19370 - 19608 + 128) >> 8 = -110 >> 8 = -1 -> 0
    # (145, 54, 34):   c 129 d -74 e -94:   R (38442 - 38446 + 128) >> 8 = 124 >> 8 = 0; G (38442 + 7400 + 19552 + 128) >> 8 = 65522 >> 8 = 255; B (38442 - 38184 + 128) >> 8 = 386 >> 8 = 1
    for (y, u, v), rgb in known.items():
        one = lambda k: np.full((1, 1), k, np.uint8)
        assert tuple(yr.convert((one(y), one(u), one(v)), 0, 0)[0, 0]) == rgb, (y, u, v)
    # chroma is replicated, not interpolated: a 3 x 3 frame under 4:2:0 takes chroma sample (y >> 1, x >> 1)
    Y = np.full((3, 3), 128, np.uint8)
    Cb, Cr = np.array([[60, 200], [128, 90]], np.uint8), np.array([[128, 40], [220, 128]], np.uint8)
    got = yr.convert((Y, Cb, Cr), 1, 1)
    for y in range(3):
        for x in range(3):
            one = lambda k: np.full((1, 1), k, np.uint8)
            assert np.array_equal(got[y, x], yr.convert((one(128), one(Cb[y >> 1, x >> 1]), one(Cr[y >> 1, x >> 1])), 0, 0)[0, 0])
    assert np.array_equal(yr.convert((Y, Cb, Cr), 1, 1, bgr=True), got[..., ::-1])


def test_the_library_converts_a_grid_of_triples_as_the_formula_does(vio):
    """Every fifth Cb and Cr (and 255) at six luma values that bracket both clips, coded as one yuv444p frame and read by the
    library: each pixel is the formula's."""
    ys = (0, 16, 17, 128, 235, 255)
    steps = np.array(list(range(0, 256, 5)) + [255], np.uint8)
    cb, cr = np.meshgrid(steps, steps)
    Y = np.concatenate([np.full(cb.shape, y, np.uint8) for y in ys])
    planes = (Y, np.tile(cb, (len(ys), 1)), np.tile(cr, (len(ys), 1)))
    p = yr.Params(pix_fmt="yuv444p", coder=0, intra=1, nh=1, nv=1)
    H, W = Y.shape
    pkt = yr.Encoder(p, W, H).encode(planes)
    got = vio.decode_frame(pkt, yr.config_record(p), W, H)
    assert np.array_equal(got, yr.convert(planes, 0, 0))
    for (y, u, v), px in zip(zip(*(a.ravel().tolist() for a in planes)), got.reshape(-1, 3).tolist()):      # the formula once more, in scalars
        c, d, e = y - 16, u - 128, v - 128
        assert px == [min(255, max(0, (298 * c + 409 * e + 128) >> 8)), min(255, max(0, (298 * c - 100 * d - 208 * e + 128) >> 8)),
                      min(255, max(0, (298 * c + 516 * d + 128) >> 8))]


# ---------------------------------------------------------------------------------------------------------------------
# the host reader on the matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", yr.MATRIX, ids=yr.case_id)
def test_the_host_reader_returns_convert_of_the_planes(vio, case):
    W, H, N, pix, coder, ec, gop, intra, sl, version = case
    planes, rgb, packets, cfg = yr.make_stream(case)
    for bgr in (False, True):
        got, pix_fmt = yr.host_read(packets, cfg, W, H, bgr=bgr)
        assert pix_fmt == pix
        assert got.shape == (N, H, W, 3) and np.array_equal(got, rgb[..., ::-1] if bgr else rgb)
        if version >= 3:                                               # the packet-to-packet decoder, the device's arbiter
            assert yr.host_stream_decode(packets, cfg, W, H, bgr=bgr).tobytes() == got.tobytes()
    if version >= 3 and gop > 1:
        with vio.StreamDecoder(cfg, W, H) as d:
            with pytest.raises(vio.VideoError, match="key frame"):
                d.decode(packets[1])


def test_pix_fmt_and_info(vio, tmp_path):
    case = (64, 48, 7, "yuv420p", 0, 1, 3, 0, (2, 2), 3)
    planes, rgb, packets, cfg = yr.make_stream(case)
    path = str(tmp_path / "y.mkv")
    with open(path, "wb") as f:
        f.write(yr.mux(packets, 64, 48, cfg))
    with vio.VideoReader(path) as r:
        assert r.pix_fmt == "yuv420p" and r.info.pix_fmt == 3
        assert (r.info.coder_type, r.info.intra, r.info.ec, r.info.slices, r.info.alpha, r.frames) == (0, 0, 1, 4, 0, 7)
        with pytest.raises(AttributeError):
            r.pix_fmt = "rgb"
        r.seek(5)                                                      # decodes forward from the key frame at 3
        assert np.array_equal(r.read(), rgb[5])
    assert vio.PIX_FMTS == ("rgb", "yuv444p", "yuv422p", "yuv420p")
    # an RGB file says so: the project's own writer, and the oracle's RGB streams
    own = str(tmp_path / "r.mkv")
    with vio.VideoWriter(own, 16, 8, 30) as w:
        w.write(np.zeros((8, 16, 3), np.uint8))
    with vio.VideoReader(own) as r:
        assert r.pix_fmt == "rgb" and r.info.pix_fmt == 0
    hdr = open(os.path.join(REPO, "include", "mdvt_video.h")).read()
    for k, name in enumerate(("RGB", "YUV444P", "YUV422P", "YUV420P")):
        assert f"MDVT_VIDEO_PIX_{name} = {k}" in hdr
    assert "BY DECREE" in hdr and "298 c + 409 e + 128" in hdr and "298 c - 100 d - 208 e + 128" in hdr and "298 c + 516 d + 128" in hdr


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _open_error(vio, tmp_path, p, W, H, packets=(b"\x00" * 16,)):
    path = str(tmp_path / "x.mkv")
    with open(path, "wb") as f:
        f.write(yr.mux(packets, W, H, yr.config_record(p)))
    with pytest.raises(vio.VideoError) as e:
        vio.VideoReader(path)
    return str(e.value)


def test_refusals_with_their_messages(vio, tmp_path):
    assert "alpha plane" in _open_error(vio, tmp_path, yr.Params(alpha=1), 34, 22)
    assert "10 bits per sample" in _open_error(vio, tmp_path, yr.Params(bits=10), 34, 22)
    assert "shifts (2, 0)" in _open_error(vio, tmp_path, yr.Params(hs=2, vs=0), 34, 22)
    assert "shifts (0, 1)" in _open_error(vio, tmp_path, yr.Params(hs=0, vs=1), 34, 22)
    assert "chroma_planes 0" in _open_error(vio, tmp_path, yr.Params(chroma_planes=0), 34, 22)
    assert "colorspace_type 2" in _open_error(vio, tmp_path, yr.Params(colorspace=2), 34, 22)
    # misaligned slice grids: the message names the grid.  33 x 21 in 2 x 2 slices has its origins at x = 33 // 2 = 16 and
    # y = 21 // 2 = 10, both on the 4:2:0 chroma grid: that stream is in the matrix and decodes.  Odd origins: 34 x 22 in 2 x 2
    # (x = 17, y = 11), 33 x 21 in 2 x 3 (y = 7) and in 4 x 1 (x = 8, 16, 24: aligned -- taken; 3 x 1: x = 11 -- refused)
    msg = _open_error(vio, tmp_path, yr.Params(pix_fmt="yuv420p", nh=2, nv=2), 34, 22)
    assert "2 x 2 slice grid" in msg and "x = 17" in msg and "34 x 22" in msg
    msg = _open_error(vio, tmp_path, yr.Params(pix_fmt="yuv420p", nh=2, nv=3), 33, 21)
    assert "2 x 3 slice grid" in msg and "y = 7" in msg
    assert "x = 11" in _open_error(vio, tmp_path, yr.Params(pix_fmt="yuv422p", nh=3, nv=1), 33, 21)
    # the codec alone and the packet-to-packet decoder refuse the same way, before anything is decoded
    cfg = yr.config_record(yr.Params(pix_fmt="yuv420p", nh=2, nv=2))
    with pytest.raises(vio.VideoError, match="2 x 2 slice grid"):
        vio.StreamDecoder(cfg, 34, 22)
    with pytest.raises(vio.VideoError, match="2 x 2 slice grid"):
        vio.decode_frame(b"\x00" * 16, cfg, 34, 22)
    # 4:2:2 subsamples columns alone: an odd y is no obstacle; 4:4:4 has no misaligned grid
    for pix, nh, nv in (("yuv422p", 1, 2), ("yuv444p", 2, 2), ("yuv444p", 3, 3)):
        p = yr.Params(pix_fmt=pix, coder=0, intra=1, nh=nh, nv=nv)
        planes = yr.planes_content(1, 21, 33, p.hs, p.vs, 4)[0]
        got = vio.decode_frame(yr.Encoder(p, 33, 21).encode(planes), yr.config_record(p), 33, 21)
        assert np.array_equal(got, yr.convert(planes, p.hs, p.vs)), (pix, nh, nv)


def test_the_class_parser_takes_the_three_formats():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    for pix in yr.PIX_FMTS:
        for coder in (0, 1):
            cfg = yr.config_record(yr.Params(pix_fmt=pix, coder=coder, intra=0, nh=2, nv=2))
            assert L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg)) is None
        cfg = yr.config_record(yr.Params(pix_fmt=pix, coder=1, intra=1))
        assert b"colorspace_type" in L.mdvt_ffv1_decode_supported(cfg, len(cfg))           # mdvt_decode_video_frames is not extended
    for kw, field in ((dict(alpha=1), b"extra_plane"), (dict(bits=10), b"bits_per_raw_sample"), (dict(hs=2, vs=0), b"log2_h_chroma_subsample"),
                      (dict(hs=0, vs=1), b"log2_v_chroma_subsample"), (dict(chroma_planes=0), b"chroma_planes"), (dict(colorspace=2), b"colorspace_type")):
        cfg = yr.config_record(yr.Params(coder=0, intra=0, **kw))
        why = L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg))
        assert why is not None and field in why, (kw, why)


def test_the_decoder_choice_treats_these_files_like_any_ffmpeg_file(vio, tmp_path, capfd):
    """`device` leaves a yuv420p file to the host with its one-line notice; `device_all` takes it to the stream decoder (no device
    is touched by the choice itself)."""
    from metric_depth_video_toolbox_amd import clip_io
    case = (64, 48, 7, "yuv420p", 0, 1, 3, 0, (2, 2), 3)
    planes, rgb, packets, cfg = yr.make_stream(case)
    path = str(tmp_path / "y.mkv")
    with open(path, "wb") as f:
        f.write(yr.mux(packets, 64, 48, cfg))
    v = clip_io.VideoFrames(path)
    assert not v.use_device_decoder("color video", "device") and not v.device_decode
    err = capfd.readouterr().err
    assert err.count("\n") == 1 and "video_decoder device: color video" in err and "decoded on the host" in err
    assert np.array_equal(np.asarray(v[2:6]), rgb[2:6])
    v.close()
    v = clip_io.VideoFrames(path)
    assert v.use_device_decoder("color video", "device_all") and v.device_decode and v.stream_decode
    got, first_out = v.read_stream_packets(4, 2)
    assert first_out == 1 and got == list(packets[3:6]) and capfd.readouterr().err == ""
    v.close()


# ---------------------------------------------------------------------------------------------------------------------
# the device decoder's core, planar mode, as a host program of its own
# ---------------------------------------------------------------------------------------------------------------------
def _check_matrix(exe):
    jobs, wants = [], []
    for case in yr.MATRIX_V3:
        W, H, N = case[:3]
        planes, rgb, packets, cfg = yr.make_stream(case)
        for order, first_out in ((0, 0), (1, N // 2), (0, N - 1)):
            jobs.append((W, H, order, first_out, cfg, list(packets)))
            wants.append((case, order, first_out, rgb))
    out = fs.run_host_program(exe, jobs)
    for (case, order, first_out, rgb), res in zip(wants, out):
        assert res is not None, yr.case_id(case)
        assert res["status"] == [0] * case[2], (yr.case_id(case), res["status"])
        assert np.array_equal(res["frames"], rgb[first_out:, ..., ::-1] if order else rgb[first_out:]), (yr.case_id(case), order, first_out)
    return out


def test_core_decodes_the_matrix_on_the_host(programs):
    plain, asan, why = programs
    out = _check_matrix(plain)                                         # (its byte accessors assert their bounds)
    golomb = [r for r, j in zip(out[::3], yr.MATRIX_V3) if j[4] == 0]
    print("counters", {k: sum(r[k] for r in golomb) for k in ("escapes", "halvings", "short_tail_runs")}, max(r["max_run_index"] for r in golomb))
    # streams that never enter the escape, the halving, a long run or a run cut by the row's end prove nothing
    assert all(r["escapes"] > 0 and r["short_tail_runs"] > 0 for r in golomb)
    assert sum(r["halvings"] for r in golomb) > 0 and max(r["max_run_index"] for r in golomb) >= 16
    # a misaligned grid is outside the class: verdict 100, as the entry point refuses it
    cfg = yr.config_record(yr.Params(pix_fmt="yuv420p", coder=0, intra=0, nh=2, nv=2))
    assert fs.run_host_program(plain, [(34, 22, 0, 0, cfg, [b"\x00" * 16])]) == [None]
    # an RGB stream through the same program takes the old rows
    frames, packets, rcfg = fs.make_stream(fs.MATRIX[9])
    res = fs.run_host_program(plain, [(fs.MATRIX[9][0], fs.MATRIX[9][1], 0, 0, rcfg, list(packets))])[0]
    assert res["status"] == [0] * len(packets) and np.array_equal(res["frames"], frames)
    if asan is None:
        pytest.skip(f"no sanitizer build: {why}")
    _check_matrix(asan)


def test_core_survives_damaged_packets(programs, vio):
    """tests/ffv1_streams.py's scheme on a yuv420p key frame.  Every run ends with a status and in-bounds accesses (asserting
    accessors, and the sanitizers where the compiler has them).  A frame the core accepts is one the host reader accepts, with the
    host's bytes; a frame the host refuses is flagged.  Where the host accepts and the core flags, the flag is BAD_SLICE_HEADER
    (slices that do not tile the frame) or NO_KEY_FRAME (the key-frame bit flipped: the host's one-packet decoder knows no run)."""
    plain, asan, why = programs
    W, H, cfg, frame, variants = yr.damage_variants()
    hosts = []
    for v in variants:
        try:
            hosts.append(vio.decode_frame(v, cfg, W, H))
        except vio.VideoError:
            hosts.append(None)
    for exe in (plain, asan):
        if exe is None:
            continue
        out = fs.run_host_program(exe, [(W, H, 0, 0, cfg, [v]) for v in variants])
        assert len(out) > 1000
        assert out[0]["status"] == [0] and np.array_equal(out[0]["frames"][0], frame)
        accepted = differ = 0
        for r, host in zip(out, hosts):
            st = r["status"][0]
            assert st in (0, 2, 3, 4, fs.NO_KEY_FRAME), st
            if host is None:
                assert st != 0, "the host refuses a frame the core accepts"
            elif st == 0:
                accepted += 1
                differ += not np.array_equal(host, frame)
                assert np.array_equal(r["frames"][0], host)
            else:
                assert st in (fs.BAD_SLICE_HEADER, fs.NO_KEY_FRAME), st
        assert [(k, out[k]["status"][0]) for k, _ in yr.DAMAGED_PICKS] == list(yr.DAMAGED_PICKS)      # the GPU test's handful
        assert accepted >= 100 and differ >= 50
    if asan is None:
        pytest.skip(f"ran with asserting accessors only; no sanitizer build: {why}")


# ---------------------------------------------------------------------------------------------------------------------
# the measurement tool's writer (tools/ffv1_ycbcr_writer.cpp: no product writer codes YCbCr)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_bench_tools_writer_is_byte_identical_to_the_reference(tmp_path):
    import shutil
    import struct
    import subprocess
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "ffv1_ycbcr_writer")
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-pthread", "-Wno-subobject-linkage", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tools", "ffv1_ycbcr_writer.cpp"), os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc_host", "mdvt_ffv1_enc.cpp")])
    raw, out = str(tmp_path / "planes.raw"), str(tmp_path / "packets.bin")
    for pix, (hs, vs) in yr.PIX_FMTS.items():
        for W, H, nh, nv in ((64, 48, 2, 2), (33, 21, 1, 1), (33, 21, 2, 2)):
            p = yr.Params(pix_fmt=pix, coder=0, intra=0, nh=nh, nv=nv)
            planes = yr.planes_content(5, H, W, hs, vs, 3)
            enc = yr.Encoder(p, W, H, gop=3)
            want = [enc.encode(pl) for pl in planes]
            with open(raw, "wb") as f:
                for pl in planes:
                    f.write(b"".join(a.tobytes() for a in pl))
            subprocess.check_call([exe, raw] + [str(v) for v in (W, H, 5, hs, vs, nh, nv, 3)] + [out])
            data = open(out, "rb").read()
            n, = struct.unpack_from("<I", data, 0)
            assert data[4:4 + n] == yr.config_record(p)
            o, got = 4 + n, []
            while o < len(data):
                n, = struct.unpack_from("<I", data, o)
                got.append(data[o + 4:o + 4 + n])
                o += 4 + n
            assert got == want, (pix, W, H, nh, nv)
    assert subprocess.run([exe, raw, "34", "22", "1", "1", "1", "2", "2", "3", out], capture_output=True).returncode == 2     # off the chroma grid


# ---------------------------------------------------------------------------------------------------------------------
# what stays unpinned: loud skips, next to tests/test_video_cpu.py::test_reader_against_ffmpeg_files
# ---------------------------------------------------------------------------------------------------------------------
def test_ffmpeg_yuv_files_decode_to_these_planes(vio):
    """Files FFmpeg itself wrote as yuv420p / yuv422p / yuv444p, with the planes it coded (tests/golden/ffv1_ffmpeg_yuv.npz: per file
    Y, Cb, Cr), through the build's reader: convert(planes)."""
    files = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "ffv1_ffmpeg_yuv*.mkv")))
    if not files:
        pytest.skip("FFV1 YCbCr INTEROPERABILITY UNPINNED: no tests/golden/ffv1_ffmpeg_yuv*.mkv -- that FFmpeg's own yuv420p files "
                    "decode to the planes this reader decodes can only be pinned where an ffmpeg exists")
    g = np.load(os.path.join(REPO, "tests", "golden", "ffv1_ffmpeg_yuv.npz"))
    for f in files:
        name = os.path.splitext(os.path.basename(f))[0]
        with vio.VideoReader(f) as r:
            hs, vs = yr.PIX_FMTS[r.pix_fmt]
            got = np.stack(list(r))
        want = np.stack([yr.convert(pl, hs, vs) for pl in zip(g[name + "_y"], g[name + "_cb"], g[name + "_cr"])])
        assert np.array_equal(got, want), f


def test_cv2_shows_these_rgb_bytes():
    """The conversion is this project's decree (BT.601 limited range, chroma replicated), not an observation of cv2.VideoCapture."""
    if not os.path.exists(os.path.join(REPO, "tests", "golden", "ffv1_cv2_yuv_frames.npz")):
        pytest.skip("YCbCr -> RGB CONVERSION UNPINNED: no tests/golden/ffv1_cv2_yuv_frames.npz -- what cv2.VideoCapture (swscale) makes of "
                    "a yuv420p FFV1 file can only be recorded where OpenCV with FFmpeg exists; the reader converts by its stated formula")
    g = np.load(os.path.join(REPO, "tests", "golden", "ffv1_cv2_yuv_frames.npz"))
    from metric_depth_video_toolbox_amd import video_io
    for f in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "ffv1_ffmpeg_yuv*.mkv"))):
        with video_io.VideoReader(f, bgr=True) as r:
            assert np.array_equal(np.stack(list(r)), g[os.path.splitext(os.path.basename(f))[0]]), f
