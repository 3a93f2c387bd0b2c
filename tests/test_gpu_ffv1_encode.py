"""The device FFV1 encoder (mdvt_encode_video_frames, ffv1_device.encode_frames_on_device) against the host encoder
(video_io.encode_frame): the same packet bytes for every frame, and the host fallback for the frames the device flags."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import torch
    from metric_depth_video_toolbox_amd import ffv1_device, video_io
    assert torch.cuda.is_available()
    return torch, ffv1_device, video_io


def _content(kind, W, H, rng, t=0):
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    if kind == "flat":
        return np.full((H, W, 3), (37, 200, 91), np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 7) & 255], -1).astype(np.uint8)
    if kind == "key":
        f = np.zeros((H, W, 3), np.uint8)
        f[..., 1] = 255
        f[H // 3:, : W // 2] = (0, 0, 0)
        return f
    if kind == "columns":                      # alternating 0 / 255: the largest differences, the quant table's 128 entry
        f = np.zeros((H, W, 3), np.uint8)
        f[:, 1::2] = 255
        f[1::2, :, 0] ^= 255
        return f
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sc = SyntheticScene(W, H, config_id=1 + t % 3, n_fg=4)
    depth_rgb, color = sc.frame(t)
    return depth_rgb if kind == "depth" else color


KINDS = ("flat", "gradient", "key", "columns", "depth", "synthetic", "noise")


def _host(video_io, frame, slices, bgr=False):
    if frame.ndim == 2:
        frame = np.repeat(frame[..., None], 3, axis=-1)
    return video_io.encode_frame(np.ascontiguousarray(frame), slices=slices, bgr=bgr, threads=8)[0]


def _device(mods, t, slices, bgr=False):
    """encode_frames_on_device's path, asserting that the device coded every frame itself (no host fallback at the defaults)."""
    torch, fd, video_io = mods
    p = fd.enqueue(fd._context(0), t, slices=slices, bgr=bgr)
    sizes = p.sizes.cpu().numpy().view(np.uint32)
    assert (sizes < fd.TOO_LARGE).all(), ("frames flagged by the device", np.nonzero(sizes >= fd.TOO_LARGE)[0].tolist())
    got = p.collect()
    assert p.host_frames == 0
    return got


def _check(mods, frames_np, slices, bgr=False, dev_frames=None):
    torch, fd, video_io = mods
    t = dev_frames if dev_frames is not None else torch.from_numpy(np.ascontiguousarray(frames_np)).cuda()
    got = _device(mods, t, slices, bgr)
    assert len(got) == len(frames_np)
    for k, f in enumerate(frames_np):
        want = _host(video_io, f, slices, bgr)
        assert got[k] == want, (f.shape, slices, k, len(got[k]), len(want))


@pytest.mark.parametrize("W,H,slices", [(1, 1, (1, 1)), (7, 5, (1, 1)), (33, 17, (4, 4)), (4, 9, (4, 4)), (7, 3, (7, 3)),
                                        (160, 90, (1, 1)), (160, 90, (4, 4)), (160, 90, (7, 3)), (160, 90, (32, 32)),
                                        (99, 61, (32, 32))])
def test_sizes_slices_contents(mods, W, H, slices):
    rng = np.random.default_rng(W * 1000 + H)
    frames = np.stack([_content(k, W, H, rng, t) for t, k in enumerate(KINDS)])
    _check(mods, frames, slices)


@pytest.mark.parametrize("W", [1920, 3840])
@pytest.mark.parametrize("slices", [(4, 4), (8, 8)])
def test_full_size_frames(mods, W, slices):
    rng = np.random.default_rng(W)
    frames = np.stack([_content(k, W, 1080, rng, 1) for k in ("depth", "synthetic", "noise")])
    _check(mods, frames, slices)


@pytest.mark.parametrize("W,slices", [(1920, (4, 4)), (1920, (8, 8)), (3840, (8, 8))])
def test_noise_batches_are_coded_on_the_device(mods, W, slices):
    """Uniform noise codes to more bytes than its raw size: the default packet buffer still holds every frame."""
    rng = np.random.default_rng(W + slices[0])
    frames = rng.integers(0, 256, (4, 1080, W, 3), dtype=np.uint8)
    _check(mods, frames, slices)


def test_bgr_grey_and_padded_layouts(mods):
    torch = mods[0]
    rng = np.random.default_rng(5)
    W, H = 97, 45
    frames = np.stack([_content(k, W, H, rng, t) for t, k in enumerate(("synthetic", "noise", "columns", "gradient"))])
    _check(mods, frames, (3, 2), bgr=True)
    # rows and frames padded: a view into a larger allocation
    big = torch.from_numpy(rng.integers(0, 256, (4, H + 3, W + 11, 3), dtype=np.uint8)).cuda()
    big[:, :H, :W] = torch.from_numpy(frames).cuda()
    view = big[:, :H, :W]
    assert not view.is_contiguous()
    _check(mods, frames, (4, 4), dev_frames=view)
    _check(mods, frames, (2, 3), bgr=True, dev_frames=view)
    # grey, dense and padded
    grey = frames[..., 1].copy()
    _check(mods, grey, (4, 4))
    gbig = torch.from_numpy(rng.integers(0, 256, (4, H + 2, W + 5), dtype=np.uint8)).cuda()
    gbig[:, :H, :W] = torch.from_numpy(grey).cuda()
    _check(mods, grey, (5, 1), dev_frames=gbig[:, :H, :W])


@pytest.mark.parametrize("n", [1, 17, 128])
def test_batches(mods, n):
    rng = np.random.default_rng(n)
    frames = np.stack([_content(KINDS[t % len(KINDS)], 64, 36, rng, t) for t in range(n)])
    _check(mods, frames, (4, 4))


def test_seeded_sweep(mods):
    torch, fd, video_io = mods
    rng = np.random.default_rng(2024)
    for case in range(300):
        W, H = int(rng.integers(1, 48)), int(rng.integers(1, 40))
        nh, nv = int(rng.integers(1, min(W, 8) + 1)), int(rng.integers(1, min(H, 8) + 1))
        n = int(rng.integers(1, 4))
        grey = rng.random() < 0.25
        bgr = bool(rng.random() < 0.5)
        kinds = [KINDS[int(rng.integers(0, len(KINDS)))] for _ in range(n)]
        frames = np.stack([_content(k, W, H, rng, t) for t, k in enumerate(kinds)])
        if grey:
            frames = frames[..., 0].copy()
        got = _device(mods, torch.from_numpy(frames).cuda(), (nh, nv), bgr)
        for k in range(n):
            assert got[k] == _host(video_io, frames[k], (nh, nv), bgr), (case, W, H, nh, nv, grey, bgr, kinds[k])


def test_independent_decoder_reads_a_device_packet(mods):
    torch, fd, video_io = mods
    from oracle import ffv1_ref as ref
    rng = np.random.default_rng(9)
    frame = _content("synthetic", 41, 23, rng, 2)
    pkt = fd.encode_frames_on_device(torch.from_numpy(frame[None].copy()).cuda(), slices=(3, 2))[0]
    p = ref.parse_config_record(video_io.encode_frame(frame, slices=(3, 2))[1])
    assert np.array_equal(ref.decode_frame_v3(pkt, p, 41, 23), frame)


def test_overflow_falls_back_to_the_host_bytes(mods):
    torch, fd, video_io = mods
    from metric_depth_video_toolbox_amd import _lib
    rng = np.random.default_rng(3)
    frames = np.stack([_content(k, 96, 64, rng, t) for t, k in enumerate(("noise", "flat", "synthetic", "noise"))])
    t = torch.from_numpy(frames).cuda()
    ctx = _lib.Context(0, 16, 16)
    # a slice capacity of 200 bytes: the noise and colour frames overflow, the flat one does not
    p = fd.enqueue(ctx, t, slices=(2, 2), slice_capacity=200)
    sizes = p.sizes.cpu().numpy().view(np.uint32)
    assert sizes[0] == fd.OVERFLOW and sizes[2] == fd.OVERFLOW and sizes[1] < fd.TOO_LARGE
    got = p.collect()
    for k in range(4):
        assert got[k] == _host(video_io, frames[k], (2, 2))
    # a packet buffer that holds only the first frame: the rest are flagged and re-encoded
    first = len(_host(video_io, frames[0], (2, 2)))
    p = fd.enqueue(ctx, t, slices=(2, 2), packets_cap=first)
    sizes = p.sizes.cpu().numpy().view(np.uint32)
    assert sizes[0] == first and all(sizes[k] == fd.OVERFLOW for k in (2, 3))
    got = p.collect()
    for k in range(4):
        assert got[k] == _host(video_io, frames[k], (2, 2))
    ctx.close()


def test_slice_past_24_bits_is_refused_like_the_host(mods):
    torch, fd, video_io = mods
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, (2160, 3840, 3), dtype=np.uint8)
    with pytest.raises(video_io.VideoError) as host_err:
        video_io.encode_frame(frame, slices=(1, 1), threads=1)
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    p = fd.enqueue(ctx, torch.from_numpy(frame[None].copy()).cuda(), slices=(1, 1))
    assert p.sizes.cpu().numpy().view(np.uint32)[0] == fd.TOO_LARGE
    with pytest.raises(video_io.VideoError) as dev_err:
        p.collect()
    assert str(dev_err.value) == str(host_err.value)
    ctx.close()


def test_device_refuses_what_the_host_refuses(mods):
    torch, fd, video_io = mods
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    L = ctx._L
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(4, dtype=torch.int64, device="cuda")
    sizes = torch.zeros(4, dtype=torch.int32, device="cuda")
    src = torch.zeros((2, 8, 40, 3), dtype=torch.uint8, device="cuda")

    def call(W=40, H=8, nh=2, nv=2, ch=3, order=0, n=2, pitch=120, stride=960):
        return L.mdvt_encode_video_frames(ctx.handle, W, H, nh, nv, C.c_void_p(src.data_ptr()), pitch, stride, ch, order, n, 0,
                                         C.c_void_p(buf.data_ptr()), buf.numel(), C.c_void_p(offs.data_ptr()),
                                         C.c_void_p(sizes.data_ptr()), None)
    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(nh=0), dict(nv=0), dict(nh=41), dict(nv=9), dict(W=2000, H=2000, nh=40, nv=40, pitch=6000, stride=12000000),
               dict(ch=2), dict(order=2), dict(n=0), dict(pitch=100), dict(stride=100)):
        assert call(**kw) == -1, kw
    ctx.close()
