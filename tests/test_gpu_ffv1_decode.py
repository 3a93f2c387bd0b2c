"""The device FFV1 decoder (mdvt_decode_video_frames, ffv1_device.decode_frames_on_device) against the host reader
(video_io.VideoReader on a file the project's writer made), and up to 250 x 61 against the independent decoder oracle/ffv1_ref.py.
Every comparison also asserts that the device decoded every frame itself (status words all zero, host_frames == 0): a frame quietly
handed to the host would make the comparison with the host empty."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    from metric_depth_video_toolbox_amd import _lib, ffv1_device, video_io
    from oracle import ffv1_ref
    assert torch.cuda.is_available()
    return torch, ffv1_device, video_io, ffv1_ref, _lib


def _content(kind, W, H, rng, t=0):
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    if kind == "constant":
        return np.full((H, W, 3), (37, 200, 91), np.uint8)
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth_rgb, color = SyntheticScene(W, H, config_id=1 + t % 3, n_fg=4).frame(t)
    return np.ascontiguousarray(depth_rgb if kind == "depth" else color)


KINDS = ("depth", "synthetic", "noise", "constant", "white")


def _file_round_trip(video_io, tmp_path, frames, slices):
    """Writes the frames with the project's writer; -> (packets, configuration record, the reader's frames, its info)."""
    H, W = frames[0].shape[:2]
    path = str(tmp_path / f"v_{W}x{H}_{slices[0]}x{slices[1]}_{len(frames)}.mkv")
    with video_io.VideoWriter(path, W, H, 30.0, slices=slices, threads=16) as w:
        for f in frames:
            w.write(np.ascontiguousarray(f))
    with video_io.VideoReader(path, threads=16) as r:
        info = r.info
        assert (info.ffv1_version, info.coder_type, info.intra, info.ec, info.slices) == (3, 1, 1, 1, slices[0] * slices[1])
        cfg = r.config_record()
        host = [r.read() for _ in frames]
        assert r.read() is None
        r.rewind()
        packets = [r.next_packet() for _ in frames]
    return packets, cfg, host, info


def _decode(mods, packets, cfg, W, H, bgr=False, out=None):
    """The device's frames as numpy, after asserting that the device decoded every one of them itself."""
    torch, fd, video_io, ref, _lib = mods
    p = fd.enqueue_decode(fd._context(0), packets, cfg, W, H, bgr=bgr, out=out)
    got = p.collect()
    assert not p.flags.any(), ("frames flagged by the device", {int(k): fd.DECODE_STATUS.get(int(p.flags[k])) for k in np.nonzero(p.flags)[0]})
    assert p.host_frames == 0
    return got.cpu().numpy()


SMALL = [(1, 1, (1, 1)), (2, 2, (2, 2)), (2, 2, (1, 1)), (17, 9, (3, 5)), (17, 9, (17, 9)), (64, 48, (4, 4)), (64, 48, (8, 8)),
         (64, 48, (1, 1)), (250, 61, (8, 8)), (250, 61, (16, 61)), (250, 61, (2, 2)), (250, 61, (7, 3)), (97, 31, (3, 5))]


@pytest.mark.parametrize("W,H,slices", SMALL)
def test_small_sizes_layouts_contents(mods, tmp_path, W, H, slices):
    torch, fd, video_io, ref, _lib = mods
    rng = np.random.default_rng(W * 1000 + H + slices[0])
    frames = [_content(k, W, H, rng, t) for t, k in enumerate(KINDS)]
    packets, cfg, host, info = _file_round_trip(video_io, tmp_path, frames, slices)
    assert fd.supported(info, cfg) is None
    for k, f in enumerate(frames):
        assert np.array_equal(host[k], f)                          # the host reader itself decodes every case
    got = _decode(mods, packets, cfg, W, H)
    for k in range(len(frames)):
        assert np.array_equal(got[k], host[k]), (W, H, slices, KINDS[k])
    got = _decode(mods, packets, cfg, W, H, bgr=True)
    for k in range(len(frames)):
        assert np.array_equal(got[k], host[k][..., ::-1]), (W, H, slices, KINDS[k], "bgr")
    # the independent decoder (pure Python: two frames per case)
    p = ref.parse_config_record(cfg)
    for k in (0, 2):
        assert np.array_equal(got[k][..., ::-1], ref.decode_frame_v3(packets[k], p, W, H)), (W, H, slices, KINDS[k], "ffv1_ref")


@pytest.mark.parametrize("W,H,slices", [(1920, 1080, (4, 4)), (1920, 1080, (16, 64)), (3840, 1080, (3, 5)), (1920, 1080, (7, 9))])
def test_large_sizes(mods, tmp_path, W, H, slices):
    torch, fd, video_io, ref, _lib = mods
    rng = np.random.default_rng(W + slices[1])
    frames = [_content(k, W, H, rng, t) for t, k in enumerate(KINDS)]
    packets, cfg, host, info = _file_round_trip(video_io, tmp_path, frames, slices)
    assert len(packets[2]) > W * H * 3                             # uniform noise codes to more than its raw size
    got = _decode(mods, packets, cfg, W, H)
    for k in range(len(frames)):
        assert np.array_equal(got[k], host[k]), (W, H, slices, KINDS[k])


@pytest.mark.parametrize("N,W,H,slices", [(1, 64, 48, (4, 4)), (16, 64, 48, (4, 4)), (16, 250, 61, (8, 8)), (1, 250, 61, (3, 5))])
def test_batches_pitches_and_views(mods, tmp_path, N, W, H, slices):
    """Distinct frames per batch; padded rows and frames; a destination view that starts at an odd byte; RGB and BGR."""
    torch, fd, video_io, ref, _lib = mods
    rng = np.random.default_rng(N * 7 + W)
    frames = [_content(KINDS[t % 3], W, H, rng, t) for t in range(N)]
    for t, f in enumerate(frames):
        f[0, 0] = (t, 255 - t, 7)                                  # no two frames alike
    packets, cfg, host, info = _file_round_trip(video_io, tmp_path, frames, slices)
    for bgr in (False, True):
        for pad, gap, base in ((0, 0, 0), (5, 0, 1), (20, 333, 3), (1, 64, 7)):
            pitch = 3 * W + pad
            stride = pitch * H + gap
            buf = torch.full((base + N * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[base:].as_strided((N, H, W, 3), (stride, pitch, 3, 1))
            got = _decode(mods, packets, cfg, W, H, bgr=bgr, out=out)
            for k in range(N):
                assert np.array_equal(got[k], host[k][..., ::-1] if bgr else host[k]), (N, W, H, bgr, pad, gap, base, k)
            # the padding, the gaps and the bytes around the view keep their fill
            flat = buf.cpu().numpy()
            mask = np.ones(flat.size, bool)
            np.lib.stride_tricks.as_strided(mask[base:], (N, H, 3 * W), (stride, pitch, 1))[...] = False
            assert (flat[mask] == 0xA5).all(), (N, W, H, pad, gap, base)


def test_128_frames_of_1080p(mods, tmp_path):
    torch, fd, video_io, ref, _lib = mods
    W, H, N = 1920, 1080, 128
    rng = np.random.default_rng(128)
    base = [_content(KINDS[t % 2], W, H, rng, t) for t in range(8)]
    frames = []
    for t in range(N):
        f = np.roll(base[t % 8], 3 * (t // 8), axis=1).copy()
        f[:4, :4] = t                                              # 128 distinct frames
        frames.append(f)
    packets, cfg, host, info = _file_round_trip(video_io, tmp_path, frames, (4, 4))
    got = _decode(mods, packets, cfg, W, H)
    for k in range(N):
        assert np.array_equal(got[k], host[k]), k


@pytest.mark.parametrize("W,H,slices", [(64, 48, (4, 4)), (160, 90, (7, 3)), (250, 61, (1, 1))])
def test_packets_of_the_device_encoder(mods, W, H, slices):
    torch, fd, video_io, ref, _lib = mods
    rng = np.random.default_rng(W)
    frames = np.stack([_content(k, W, H, rng, t) for t, k in enumerate(KINDS)])
    packets = fd.encode_frames_on_device(torch.from_numpy(frames).cuda(), slices=slices)
    cfg = video_io.encode_frame(frames[0], slices=slices)[1]
    got = _decode(mods, packets, cfg, W, H)
    assert np.array_equal(got, frames)
    for k in range(len(frames)):
        assert np.array_equal(video_io.decode_frame(packets[k], cfg, W, H), frames[k])


@pytest.mark.parametrize("ec", [1, 0])
@pytest.mark.parametrize("W,H,nh,nv,micro", [(40, 22, 2, 2, 4), (40, 22, 1, 1, 4), (97, 31, 3, 2, 3), (250, 61, 8, 8, 4), (17, 9, 3, 5, 4)])
def test_packets_of_the_independent_encoder(mods, W, H, nh, nv, micro, ec):
    """oracle/ffv1_ref.py's encoder in the in-class modes: the only source of packets without CRCs (ec 0)."""
    torch, fd, video_io, ref, _lib = mods
    rng = np.random.default_rng(W + ec)
    frames = [_content(k, W, H, rng, t) for t, k in enumerate(KINDS)]
    p = ref.Params(nh=nh, nv=nv, ec=ec, micro=micro)
    enc = ref.StreamEncoder(p, W, H)
    packets = [enc.encode(f) for f in frames]
    cfg = ref.config_record(p)
    got = _decode(mods, packets, cfg, W, H)
    for k, f in enumerate(frames):
        assert np.array_equal(video_io.decode_frame(packets[k], cfg, W, H), f)            # the host reader decodes it
        assert np.array_equal(got[k], f), (W, H, nh, nv, ec, KINDS[k])


def _custom_table(ref):
    one = list(ref.DEFAULT_ONE)
    for i in range(20, 200, 7):
        one[i] = min(248, one[i] + 3)
    return one


OUT_OF_CLASS = [(dict(coder=0), "coder_type"), (dict(intra=0), "intra"), (dict(version=1), "version"), (dict(version=0, coder=0), "version"),
                (dict(alpha=1), "extra_plane"), (dict(coder=2, custom=True), "coder_type"), (dict(five=True), "quantisation tables"),
                (dict(coder=0, intra=0, nh=2, nv=2), "coder_type")]


def test_out_of_class_streams_are_refused_and_nothing_is_written(mods):
    torch, fd, video_io, ref, _lib = mods
    W, H, N = 40, 22, 2
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    rng = np.random.default_rng(5)
    try:
        for kw, field in OUT_OF_CLASS:
            kw = dict(kw)
            if kw.pop("custom", False):
                kw["custom"] = _custom_table(ref)
            p = ref.Params(**kw)
            frames = [rng.integers(0, 256, (H, W, 4 if p.alpha else 3), dtype=np.uint8) for _ in range(N)]
            enc = ref.StreamEncoder(p, W, H, gop=1 if p.intra else 2)
            packets = [enc.encode(f) for f in frames]
            cfg = ref.config_record(p)
            blob = torch.from_numpy(np.frombuffer(b"".join(packets), np.uint8).copy()).cuda()
            sizes = torch.tensor([len(x) for x in packets], dtype=torch.int32, device="cuda")
            offs = torch.tensor([0, len(packets[0])], dtype=torch.int64, device="cuda")
            dst = torch.full((N, H, W, 3), 0x5C, dtype=torch.uint8, device="cuda")
            status = torch.full((N,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
            rc = L.mdvt_decode_video_frames(ctx.handle, W, H, cfg, len(cfg), C.c_void_p(blob.data_ptr()), blob.numel(),
                                            C.c_void_p(offs.data_ptr()), C.c_void_p(sizes.data_ptr()), N, C.c_void_p(dst.data_ptr()),
                                            3 * W, 3 * W * H, 0, C.c_void_p(status.data_ptr()), None)
            torch.cuda.synchronize()
            text = (L.mdvt_last_error(ctx.handle) or b"").decode()
            assert rc == -3, (kw, rc, text)                                      # MDVT_ERR_UNSUPPORTED
            assert field in text, (kw, text)
            assert (dst.cpu().numpy() == 0x5C).all() and (status.cpu().numpy() == 0x5C5C5C5C).all(), kw
            with pytest.raises(_lib.MdvtError) as e:
                fd.decode_frames_on_device(packets, cfg, W, H)
            assert e.value.code == -3 and field in str(e.value)
        # the context decodes a good batch afterwards
        good = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3)]
        pk = [video_io.encode_frame(f, slices=(2, 2)) for f in good]
        p = fd.enqueue_decode(ctx, [x[0] for x in pk], pk[0][1], W, H)
        got = p.collect().cpu().numpy()
        assert p.host_frames == 0 and all(np.array_equal(got[k], good[k]) for k in range(3))
    finally:
        ctx.close()


def test_bad_arguments(mods):
    torch, fd, video_io, ref, _lib = mods
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    W, H = 8, 4
    pkt, cfg = video_io.encode_frame(np.zeros((H, W, 3), np.uint8), slices=(1, 1))
    blob = torch.from_numpy(np.frombuffer(pkt, np.uint8).copy()).cuda()
    sizes = torch.tensor([len(pkt), len(pkt)], dtype=torch.int32, device="cuda")
    offs = torch.zeros(2, dtype=torch.int64, device="cuda")
    dst = torch.full((2, H, W, 3), 0x5C, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())

    def call(cfg_=cfg, packets=vp(blob), o=vp(offs), s=vp(sizes), n=2, d=vp(dst), pitch=3 * W, stride=3 * W * H, order=0, st=vp(status)):
        return L.mdvt_decode_video_frames(ctx.handle, W, H, cfg_, len(cfg) if cfg_ else 0, packets, blob.numel(), o, s, n, d, pitch, stride, order, st, None)
    try:
        for kw in (dict(cfg_=None), dict(packets=None), dict(o=None), dict(s=None), dict(d=None), dict(st=None), dict(n=0), dict(pitch=3 * W - 1),
                   dict(stride=3 * W * H - 1), dict(order=2)):
            assert call(**kw) == -1, kw                                          # MDVT_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 0x5C).all() and (status.cpu().numpy() == 0x5C5C5C5C).all()
        assert call() == 0
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all() and (dst.cpu().numpy() == 0).all()
    finally:
        ctx.close()


def test_damage_caught_before_the_range_decoder(mods):
    """One batch, once: a flipped payload bit (CRC), a slice size that points outside the packet, a truncated packet and stray bytes
    before the first slice.  Those frames and only those are flagged, their neighbours are exact, and the wrapper then raises the
    host's VideoError for them."""
    torch, fd, video_io, ref, _lib = mods
    W, H, slices = 64, 48, (4, 4)
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(7)]
    pk = [video_io.encode_frame(f, slices=slices) for f in frames]
    cfg = pk[0][1]
    packets = [bytearray(p[0]) for p in pk]
    packets[1][len(packets[1]) // 2] ^= 0x10                                     # a payload bit of some slice
    packets[3][-8:-5] = b"\xff\xff\xff"                                          # the last slice claims 2^24 - 1 bytes
    packets[4] = packets[4][:-9]                                                 # truncated
    packets[5] = bytearray(b"\x00\x01\x02") + packets[5]                         # stray bytes before the first slice
    packets = [bytes(p) for p in packets]
    want = {1: 1, 3: 4, 4: 4, 5: 4}
    for k in want:                                                               # the host refuses exactly these
        with pytest.raises(video_io.VideoError):
            video_io.decode_frame(packets[k], cfg, W, H)
    p = fd.enqueue_decode(fd._context(0), packets, cfg, W, H)
    p.done.synchronize()
    flags = p.status.cpu().numpy().view(np.uint32)
    assert {int(k): int(flags[k]) for k in np.nonzero(flags)[0]} == want
    got = p.out.cpu().numpy()
    for k in (0, 2, 6):
        assert np.array_equal(got[k], frames[k]), k
    with pytest.raises(video_io.VideoError):
        p.collect()
    assert p.host_frames == 1                                                    # the first flagged frame went to the host, which refused it
