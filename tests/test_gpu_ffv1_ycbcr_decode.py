"""mdvt_decode_video_stream (include/mdvt_ffv1_stream_decode.h) on YCbCr streams -- yuv444p, yuv422p, yuv420p -- on the GPU: the
version 3 streams of tests/ffv1_ycbcr_ref.py's matrix equal the packet-to-packet host decoder (video_io.StreamDecoder, the device's
arbiter) byte for byte, which equals convert(planes) (tests/test_ffv1_ycbcr_cpu.py).  No comparison here may pass by routing frames
to the host: every one asserts all-zero status words and host_frames == 0."""
import ctypes as C

import numpy as np
import pytest

import ffv1_streams as fs
import ffv1_ycbcr_ref as yr

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3


@pytest.fixture(scope="module")
def mods():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, ffv1_device, video_io
    return torch, ffv1_device, video_io, _lib


def _decode(mods, packets, cfg, W, H, **kw):
    torch, fd, video_io, _lib = mods
    p = fd.enqueue_decode_stream(_lib.shared_context(0), list(packets), cfg, W, H, **kw)
    out = p.collect()
    torch.cuda.synchronize()
    assert p.host_frames == 0 and not p.flags.any(), (p.host_frames, p.flags)
    return out.cpu().numpy()


@pytest.mark.parametrize("case", yr.MATRIX_V3, ids=yr.case_id)
def test_the_matrix(mods, case):
    W, H, N, pix, coder, ec, gop, intra, sl, version = case
    planes, rgb, packets, cfg = yr.make_stream(case)
    host = {bgr: yr.host_stream_decode(packets, cfg, W, H, bgr=bgr) for bgr in (False, True)}
    assert np.array_equal(host[False], rgb) and np.array_equal(host[True], rgb[..., ::-1])
    # first_out at 0, inside a run (the frame behind the last key frame), on a key frame and at the last packet; both orders
    keys = [t for t in range(N) if t % gop == 0]
    for first_out in sorted({0, 1, min(N - 1, keys[-1] + 1), keys[-1], N - 1}):
        for bgr in (False, True):
            got = _decode(mods, packets, cfg, W, H, first_out=first_out, bgr=bgr)
            assert got.tobytes() == host[bgr][first_out:].tobytes(), (first_out, bgr)


@pytest.mark.parametrize("pix", list(yr.PIX_FMTS))
def test_padded_pitch_and_stride_in_a_poisoned_arena(mods, pix):
    """Padded rows and frames, a destination that starts at an odd byte, first_out inside a run: nothing but the first 3 * W bytes of
    the stored rows changes (the luma and Cb rows that wait for their Cr stay inside them), on a poison and on its complement."""
    torch = mods[0]
    for case in ((64, 48, 7, pix, 0, 1, 3, 0, (2, 2), 3), (33, 21, 7, pix, 1, 1, 3, 0, (1, 1), 3)):
        assert case in yr.MATRIX_V3
        W, H, N = case[:3]
        planes, rgb, packets, cfg = yr.make_stream(case)
        first_out = 1
        n = N - first_out
        for poison in (0xA5, 0x5A):
            for bgr, pad, gap, base in ((False, 0, 0, 0), (True, 5, 0, 1), (False, 20, 333, 3), (True, 1, 64, 7)):
                pitch = 3 * W + pad
                stride = pitch * H + gap
                buf = torch.full((base + n * stride + 64,), poison, dtype=torch.uint8, device="cuda")
                out = buf[base:].as_strided((n, H, W, 3), (stride, pitch, 3, 1))
                got = _decode(mods, packets, cfg, W, H, first_out=first_out, bgr=bgr, out=out)
                assert np.array_equal(got, rgb[first_out:, ..., ::-1] if bgr else rgb[first_out:]), (poison, bgr, pad, gap, base)
                flat = buf.cpu().numpy()
                mask = np.ones(flat.size, bool)
                np.lib.stride_tricks.as_strided(mask[base:], (n, H, 3 * W), (stride, pitch, 1))[...] = False
                assert (flat[mask] == poison).all(), (poison, pad, gap, base)


def test_a_call_holding_two_key_frame_runs(mods):
    """Frames 2 .. 5 of a gop 3 stream: the tail of one run, decoded from its key frame for the state alone, and a whole second run."""
    case = (64, 48, 7, "yuv420p", 0, 1, 3, 0, (2, 2), 3)
    W, H = case[:2]
    planes, rgb, packets, cfg = yr.make_stream(case)
    got = _decode(mods, packets[:6], cfg, W, H, first_out=2)
    assert np.array_equal(got, rgb[2:6])


def test_a_crc_flip_breaks_its_run_alone(mods):
    torch, fd, video_io, _lib = mods
    case = (64, 48, 7, "yuv420p", 0, 1, 3, 0, (2, 2), 3)              # ec 1; keys at 0, 3, 6
    W, H, N = case[:3]
    planes, rgb, packets, cfg = yr.make_stream(case)
    flipped = list(packets)
    b = bytearray(flipped[3]); b[len(b) // 2] ^= 0x10; flipped[3] = bytes(b)
    p = fd.enqueue_decode_stream(_lib.shared_context(0), flipped, cfg, W, H)
    p.done.synchronize()
    flags = p.status.cpu().numpy().view(np.uint32).tolist()
    assert flags == [0, 0, 0, fs.CRC_MISMATCH, fs.BROKEN_RUN, fs.BROKEN_RUN, 0]
    got = p.out.cpu().numpy()
    assert np.array_equal(got[:3], rgb[:3]) and np.array_equal(got[6], rgb[6])
    with pytest.raises(video_io.VideoError, match="CRC"):              # the host refuses the run as well
        p.collect()


def test_a_misaligned_slice_grid_is_refused_with_nothing_written(mods):
    """A slice origin off the chroma grid: 34 x 22 in 2 x 2 slices under 4:2:0 (x = 17, y = 11), in 2 x 1 under 4:2:2 (x = 17), and
    33 x 21 in 2 x 3 under 4:2:0 (y = 7).  MDVT_ERR_UNSUPPORTED names the slice grid; neither the frames nor the status words are
    touched.  (The packets are never looked at: any bytes do.)  33 x 21 in 2 x 2 slices has its origins at x = 16 and y = 10: that
    grid is aligned and decodes, in the matrix."""
    torch, fd, video_io, _lib = mods
    L = _lib.load()
    ctx = _lib.shared_context(0)
    for W, H, pix, nh, nv in ((34, 22, "yuv420p", 2, 2), (34, 22, "yuv422p", 2, 1), (33, 21, "yuv420p", 2, 3)):
        cfg = yr.config_record(yr.Params(pix_fmt=pix, coder=0, intra=0, nh=nh, nv=nv))
        assert L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg)) is None          # the record alone is in the class
        blob = torch.zeros(64, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(2, dtype=torch.int64, device="cuda")
        sizes = torch.full((2,), 32, dtype=torch.int32, device="cuda")
        dst = torch.full((2, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rc = L.mdvt_decode_video_stream(ctx.handle, W, H, cfg, len(cfg), C.c_void_p(blob.data_ptr()), 64, C.c_void_p(offs.data_ptr()),
                                        C.c_void_p(sizes.data_ptr()), 2, 0, C.c_void_p(dst.data_ptr()), 3 * W, 3 * W * H, 0,
                                        C.c_void_p(status.data_ptr()), None)
        assert rc == UNSUPPORTED
        with pytest.raises(_lib.MdvtError, match=f"{nh} x {nv} slice grid"):
            ctx.check(rc)
        torch.cuda.synchronize()
        assert (dst == 0xA5).all() and (status == 0x5A5A5A5A).all()
    # the same frame sizes in aligned grids decode (the matrix); 4:4:4 has no misaligned grid
    cfg = yr.config_record(yr.Params(pix_fmt="yuv444p", coder=0, intra=0, nh=2, nv=2))
    p = yr.Params(pix_fmt="yuv444p", coder=0, intra=0, nh=2, nv=2)
    planes = yr.planes_content(2, 21, 33, 0, 0, 3)
    enc = yr.Encoder(p, 33, 21, gop=2)
    got = _decode(mods, [enc.encode(pl) for pl in planes], cfg, 33, 21)
    assert np.array_equal(got, np.stack([yr.convert(pl, 0, 0) for pl in planes]))


def test_supported_names_the_field(mods):
    torch, fd, video_io, _lib = mods
    L = _lib.load()
    for pix in yr.PIX_FMTS:
        for coder in (0, 1):
            cfg = yr.config_record(yr.Params(pix_fmt=pix, coder=coder, intra=0, nh=2, nv=2))
            assert L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg)) is None
        cfg = yr.config_record(yr.Params(pix_fmt=pix, coder=1, intra=1, nh=2, nv=2))
        assert b"colorspace_type" in L.mdvt_ffv1_decode_supported(cfg, len(cfg))           # the intra decoder's class stays RGB
    for kw, field in ((dict(alpha=1), b"extra_plane"), (dict(bits=10), b"bits_per_raw_sample"), (dict(hs=2, vs=0), b"log2_h_chroma_subsample"),
                      (dict(hs=0, vs=1), b"log2_v_chroma_subsample"), (dict(chroma_planes=0), b"chroma_planes"), (dict(colorspace=2), b"colorspace_type")):
        cfg = yr.config_record(yr.Params(coder=0, intra=0, **kw))
        why = L.mdvt_ffv1_stream_decode_supported(cfg, len(cfg))
        assert why is not None and field in why, (kw, why)
        with pytest.raises(_lib.MdvtError, match=field.decode()):
            fd.enqueue_decode_stream(_lib.shared_context(0), [b"\x00" * 8], cfg, 16, 8)


def test_an_rgb_stream_before_and_after_a_ycbcr_stream_on_one_context(mods):
    torch, fd, video_io, _lib = mods
    ctx = _lib.Context(0, 16, 16)
    try:
        def run(packets, cfg, W, H):
            p = fd.enqueue_decode_stream(ctx, list(packets), cfg, W, H)
            out = p.collect().cpu().numpy()
            assert p.host_frames == 0 and not p.flags.any()
            return out
        seen = []
        for rgb_case in (fs.COUNTERS_CASE, fs.MATRIX[1]):               # Golomb-Rice and range coder, 67 x 37 in 3 x 2 slices
            frames, packets, cfg = fs.make_stream(rgb_case)
            before = run(packets, cfg, rgb_case[0], rgb_case[1])
            assert np.array_equal(before, frames)
            for case in ((64, 48, 7, "yuv420p", rgb_case[3], 1, 3, 0, (2, 2), 3), (33, 21, 7, "yuv422p", rgb_case[3], 1, 3, 0, (1, 1), 3)):
                planes, rgb, ypackets, ycfg = yr.make_stream(case)
                assert np.array_equal(run(ypackets, ycfg, case[0], case[1]), rgb)
            after = run(packets, cfg, rgb_case[0], rgb_case[1])
            assert after.tobytes() == before.tobytes()
            seen.append(rgb_case[3])
        assert seen == [0, 1]
    finally:
        ctx.close()


def test_damaged_packets_end_in_the_cpu_runs_status(mods):
    """A fixed handful of the damaged YCbCr packets the CPU run decoded cleanly to a status (yr.DAMAGED_PICKS: the same core with
    asserting accessors and under the sanitizers, pinned by tests/test_ffv1_ycbcr_cpu.py): the same status here, and the host's
    bytes where the status is 0."""
    torch, fd, video_io, _lib = mods
    W, H, cfg, frame, variants = yr.damage_variants()
    for k, want in yr.DAMAGED_PICKS:
        v = variants[k]
        p = fd.enqueue_decode_stream(_lib.shared_context(0), [v], cfg, W, H)
        p.done.synchronize()
        st = int(p.status.cpu().numpy().view(np.uint32)[0])
        assert st == want, (k, len(v), st, want)
        if st == 0:
            assert np.array_equal(p.out[0].cpu().numpy(), video_io.decode_frame(v, cfg, W, H)), k
