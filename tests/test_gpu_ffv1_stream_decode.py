"""mdvt_decode_video_stream (include/mdvt_ffv1_stream_decode.h) on the GPU: the stream matrix of tests/ffv1_streams.py -- Golomb-Rice
and range coder, inter frames, every gop, slice grid and size -- equals the source frames, which are what the host reader reads
(tests/test_video_stream_decoder_cpu.py::test_the_matrix_streams_are_what_the_host_reader_reads).  No comparison here may pass by
routing frames to the host: every one asserts all-zero status words and host_frames == 0."""
import numpy as np
import pytest

import ffv1_streams as fs

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("case", fs.MATRIX, ids=fs.case_id)
def test_the_matrix(mods, case):
    W, H, N, coder, ec, gop, intra, sl = case
    frames, packets, cfg = fs.make_stream(case)
    keys = [t for t in range(N) if t % gop == 0]
    # first_out at 0, inside a run, on a key frame and at the last packet
    for first_out in sorted({0, min(N - 1, keys[-1] + 1), keys[-1], N - 1}):
        for bgr in (False, True):
            got = _decode(mods, packets, cfg, W, H, first_out=first_out, bgr=bgr)
            assert np.array_equal(got, frames[first_out:, ..., ::-1] if bgr else frames[first_out:]), (first_out, bgr)


def test_both_entry_points_decode_an_intra_stream_alike(mods):
    """The coder 1, intra = 1 stream of the matrix (67x37, 2 frames, 3x2 slices) is in both classes: mdvt_decode_video_frames and
    mdvt_decode_video_stream (first_out 0 and 1) give the source frames, with all-zero status words and nothing left to the host."""
    torch, fd, video_io, _lib = mods
    case = (67, 37, 2, 1, 1, 1, 1, (3, 2))
    assert case in fs.MATRIX
    W, H, N = case[:3]
    frames, packets, cfg = fs.make_stream(case)
    p = fd.enqueue_decode(_lib.shared_context(0), list(packets), cfg, W, H)
    intra = p.collect().cpu().numpy()
    assert p.host_frames == 0 and p.flags.tolist() == [0] * N
    assert np.array_equal(intra, frames)
    for first_out in (0, 1):
        got, flags, host_frames = fd.decode_stream_on_device(list(packets), cfg, W, H, first_out=first_out)
        assert host_frames == 0 and flags.tolist() == [0] * N
        got = got.cpu().numpy()
        assert np.array_equal(got, frames[first_out:]) and got.tobytes() == intra[first_out:].tobytes()
    got, flags = fd.decode_frames_on_device(list(packets), cfg, W, H)
    assert flags.tolist() == [0] * N and np.array_equal(got.cpu().numpy(), frames)


def test_the_host_reader_agrees_on_the_gpu_machine(mods):
    case = fs.COUNTERS_CASE
    frames, packets, cfg = fs.make_stream(case)
    host, err = fs.host_read(packets, cfg, case[0], case[1])
    assert err is None and np.array_equal(np.stack(host), frames)


def test_a_call_whose_first_packet_is_no_key_frame(mods):
    torch, fd, video_io, _lib = mods
    case = fs.COUNTERS_CASE                                            # keys at 0, 3, 6
    W, H, N = case[:3]
    frames, packets, cfg = fs.make_stream(case)
    for skip in (1, 2):
        p = fd.enqueue_decode_stream(_lib.shared_context(0), list(packets[skip:]), cfg, W, H)
        p.done.synchronize()
        flags = p.status.cpu().numpy().view(np.uint32)
        assert flags.tolist() == [fd.NO_KEY_FRAME] * (3 - skip) + [0] * 4
        assert np.array_equal(p.out[3 - skip:].cpu().numpy(), frames[3:])
        # collect() cannot decode the frames in front of the key frame either: the host's own refusal
        with pytest.raises(video_io.VideoError, match="key frame"):
            p.collect()


def test_padded_pitches_strides_and_an_odd_base(mods):
    """Padded rows and frames; a destination view that starts at an odd byte; RGB and BGR; the fill around the view stays."""
    torch = mods[0]
    for case in (fs.COUNTERS_CASE, fs.MATRIX[9]):
        W, H, N = case[:3]
        frames, packets, cfg = fs.make_stream(case)
        first_out = 1
        n = N - first_out
        for bgr in (False, True):
            for pad, gap, base in ((0, 0, 0), (5, 0, 1), (20, 333, 3), (1, 64, 7)):
                pitch = 3 * W + pad
                stride = pitch * H + gap
                buf = torch.full((base + n * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                out = buf[base:].as_strided((n, H, W, 3), (stride, pitch, 3, 1))
                got = _decode(mods, packets, cfg, W, H, first_out=first_out, bgr=bgr, out=out)
                assert np.array_equal(got, frames[first_out:, ..., ::-1] if bgr else frames[first_out:]), (bgr, pad, gap, base)
                flat = buf.cpu().numpy()
                mask = np.ones(flat.size, bool)
                np.lib.stride_tricks.as_strided(mask[base:], (n, H, 3 * W), (stride, pitch, 1))[...] = False
                assert (flat[mask] == 0xA5).all(), (pad, gap, base)


def test_1080p_from_the_stream_writer(mods, tmp_path):
    """13 frames of 1920 x 1080, 4 x 4 slices, a key frame every 12, written by video_io.VideoWriter(coder=0): against the host reader."""
    torch, fd, video_io, _lib = mods
    W, H, N = 1920, 1080, 13
    base = fs.stream_content(2, H, W, 1080)
    path = str(tmp_path / "big.mkv")
    with video_io.VideoWriter(path, W, H, 24, slices=(4, 4), coder=0, gop=12) as w:
        for t in range(N):
            f = np.roll(base[t % 2], 5 * t, axis=1)
            f[:4, :4] = t
            w.write(np.ascontiguousarray(f))
    with video_io.VideoReader(path) as r:
        cfg = r.config_record()
        packets = [r.next_packet() for _ in range(N)]
    assert [fd.packet_is_key(p) for p in packets] == [t % 12 == 0 for t in range(N)]
    with video_io.VideoReader(path) as r:
        host = np.stack(list(r))
    got = _decode(mods, packets, cfg, W, H)
    assert np.array_equal(got, host)


def test_damaged_packets_end_in_the_cpu_runs_status(mods):
    """A fixed handful of the damaged packets the CPU run decoded cleanly to a status (fs.DAMAGED_PICKS: the same core with
    asserting accessors and under the sanitizers, pinned by tests/test_video_stream_decoder_cpu.py): the same status here, and
    the host's bytes where the status is 0."""
    torch, fd, video_io, _lib = mods
    W, H, cfg, picks = fs.damaged_picks()
    for v, want in picks:
        p = fd.enqueue_decode_stream(_lib.shared_context(0), [v], cfg, W, H)
        p.done.synchronize()
        st = int(p.status.cpu().numpy().view(np.uint32)[0])
        assert st == want, (len(v), st, want)
        if st == 0:
            assert np.array_equal(p.out[0].cpu().numpy(), video_io.decode_frame(v, cfg, W, H))


def test_a_crc_flip_breaks_its_run_alone(mods):
    torch, fd, video_io, _lib = mods
    case = fs.COUNTERS_CASE                                            # ec 1; keys at 0, 3, 6
    W, H, N = case[:3]
    frames, packets, cfg = fs.make_stream(case)
    flipped = list(packets)
    b = bytearray(flipped[3]); b[len(b) // 2] ^= 0x10; flipped[3] = bytes(b)
    p = fd.enqueue_decode_stream(_lib.shared_context(0), flipped, cfg, W, H)
    p.done.synchronize()
    flags = p.status.cpu().numpy().view(np.uint32).tolist()
    assert flags == [0, 0, 0, fs.CRC_MISMATCH, fs.BROKEN_RUN, fs.BROKEN_RUN, 0]
    got = p.out.cpu().numpy()
    assert np.array_equal(got[:3], frames[:3]) and np.array_equal(got[6], frames[6])
    with pytest.raises(video_io.VideoError, match="CRC"):              # the host refuses the run as well
        p.collect()
    # an intact copy of the same call: collect() has nothing to do
    assert np.array_equal(_decode(mods, packets, cfg, W, H), frames)


def test_refused_arguments(mods):
    torch, fd, video_io, _lib = mods
    from oracle import ffv1_ref as ref
    case = fs.MATRIX[9]
    W, H, N = case[:3]
    frames, packets, cfg = fs.make_stream(case)
    ctx = _lib.shared_context(0)
    for first_out in (-1, N):
        with pytest.raises(ValueError, match="first_out"):
            fd.enqueue_decode_stream(ctx, list(packets), cfg, W, H, first_out=first_out)
    with pytest.raises(_lib.MdvtError, match="extra_plane"):
        fd.enqueue_decode_stream(ctx, list(packets), ref.config_record(ref.Params(alpha=1)), W, H)
