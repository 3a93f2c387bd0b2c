"""mdvt_convergence_depths (include/mdvt_convergence.h) and find_convergence_depth.convergence_depths against NumPy on the test
machine (tests/convergence_ref.py: the reference's own lines): the float32 mean of every frame bit for bit -- `==`, or both NaN; no
tolerance -- at every size where the order of summation can go wrong, with masks of every count around the order's thresholds,
both byte orders, padded layouts, launch sets, streams and every refusal."""
import ctypes as C

import numpy as np
import pytest

import convergence_ref as cr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def mods():
    import torch
    from metric_depth_video_toolbox_amd import _lib, find_convergence_depth as fcd
    return torch, _lib, fcd


def _check(got, want, what):
    bad = cr.same_bits(got, want)
    print(f"{what}: {len(bad)} mismatches of {len(want)}")
    assert bad.size == 0, (f"{what}: {len(bad)} of {len(want)} means differ; first at frame {bad[0]}: "
                           f"got {np.asarray(got)[bad[0]]!r} ({np.asarray(got, np.float32)[bad[0]].tobytes().hex()}), "
                           f"want {want[bad[0]]!r} ({want[bad[0]].tobytes().hex()})")


# W x H, n = W * H: where the order can go wrong
SIZES = [(5, 1), (13, 9), (16, 8), (13, 10), (128, 64), (205, 40), (257, 33), (171, 96), (640, 480), (1024, 540), (1920, 1080)]


@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_unmasked_frame_equals_numpy(mods, W, H):
    torch, _lib, fcd = mods
    rng = np.random.default_rng(W * 10007 + H)
    depth = cr.random_depth(rng, 1, H, W)
    want, n = cr.clip_means(depth)
    means, counts = fcd.convergence_depths(torch.from_numpy(depth).cuda(), counts=True)
    _check(means.cpu().numpy(), want, f"unmasked {W}x{H}")
    assert counts.cpu().numpy().tolist() == n.tolist() == [W * H]


@pytest.mark.parametrize("max_depth", [100, 20, 255])
def test_max_depths_and_byte_orders(mods, max_depth):
    torch, _lib, fcd = mods
    rng = np.random.default_rng(max_depth)
    for W, H in ((257, 33), (171, 96), (128, 64)):
        depth = cr.random_depth(rng, 2, H, W)
        mask = np.repeat(rng.choice(np.array([0, 255], np.uint8), (1, H, W, 1), p=(0.4, 0.6)), 3, axis=3)
        mask[..., 1] = np.where(mask[..., 1] == 255, rng.integers(200, 256, (1, H, W), dtype=np.uint8), 0)     # coloured: R and B matter
        want, n = cr.clip_means(depth, mask, max_depth)
        for bgr in (False, True):
            d = torch.from_numpy(np.ascontiguousarray(depth[..., ::-1]) if bgr else depth).cuda()
            m = torch.from_numpy(np.ascontiguousarray(mask[..., ::-1]) if bgr else mask).cuda()
            means, counts = fcd.convergence_depths(d, m, max_depth, bgr=bgr, counts=True)
            _check(means.cpu().numpy(), want, f"{W}x{H} max_depth {max_depth} bgr={bgr}")
            assert counts.cpu().numpy().tolist() == n.tolist()


def _padded(torch, frames, pitch, stride, base, poison):
    """The frames inside a poisoned byte buffer at `base`, rows `pitch` and frames `stride` bytes apart: a strided view of it."""
    N, H, W, _ = frames.shape
    buf = torch.full((base + N * stride + 64,), poison, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (N, H, W, 3), (stride, pitch, 3, 1), base)
    view.copy_(torch.from_numpy(frames).cuda())
    return view


@pytest.mark.parametrize("W,H,pad,gap,base", [(171, 96, 1, 5, 1), (171, 96, 3, 0, 0), (172, 50, 4, 8, 4), (172, 50, 20, 64, 8),
                                              (172, 50, 2, 0, 0), (172, 50, 4, 0, 2), (256, 40, 0, 0, 0)])
def test_padded_pitches_and_strides_with_poisoned_padding(mods, W, H, pad, gap, base):
    torch, _lib, fcd = mods
    rng = np.random.default_rng(W + pad * 7 + gap)
    N = 3
    depth = cr.random_depth(rng, N, H, W)
    mask = np.repeat(rng.choice(np.array([0, 240, 241, 255], np.uint8), (2, H, W, 1)), 3, axis=3)
    want, n = cr.clip_means(depth, mask)
    pitch = 3 * W + pad
    stride = H * pitch + gap
    for poison in (0xFF, 0x00, 0xF1):                                # (0xF1 three times is a selected grey: padding read as pixels would show)
        d = _padded(torch, depth, pitch, stride, 256 + base, poison)
        m = _padded(torch, mask, pitch, stride, 256 + base, poison)
        means, counts = fcd.convergence_depths(d, m, counts=True)
        _check(means.cpu().numpy(), want, f"{W}x{H} pad {pad} gap {gap} base {base} poison {poison:#x}")
        assert counts.cpu().numpy().tolist() == n.tolist()


COUNTS = (0, 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 16387)


def test_masked_counts_around_every_threshold_of_the_order(mods):
    """171 x 96: each count placed as the first m pixels, as the last m pixels and at seeded random positions -- one call."""
    torch, _lib, fcd = mods
    W, H = 171, 96
    rng = np.random.default_rng(171)
    sel = np.zeros((len(COUNTS) * 3, H * W), bool)
    for i, m in enumerate(COUNTS):
        sel[3 * i, :m] = True
        sel[3 * i + 1, H * W - m:] = True
        sel[3 * i + 2, rng.choice(H * W, m, replace=False)] = True
    N = len(sel)
    # white (255) or, here and there, just white enough (241) where selected; black or just not white enough (240) elsewhere
    on = rng.choice(np.array([255, 241], np.uint8), (N, H * W), p=(0.8, 0.2))
    off = rng.choice(np.array([0, 240], np.uint8), (N, H * W), p=(0.8, 0.2))
    mask = np.repeat(np.where(sel, on, off).reshape(N, H, W, 1), 3, axis=3)
    depth = cr.random_depth(rng, N, H, W)
    want, n = cr.clip_means(depth, mask)
    assert n.tolist() == [m for m in COUNTS for _ in range(3)]
    means, counts = fcd.convergence_depths(torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda(), counts=True)
    _check(means.cpu().numpy(), want, "masked counts 171x96")
    assert counts.cpu().numpy().tolist() == n.tolist()
    assert np.isnan(means.cpu().numpy()[:3]).all()


def test_the_threshold_and_coloured_mask_pixels(mods):
    torch, _lib, fcd = mods
    W, H = 64, 48
    rng = np.random.default_rng(240)
    depth = cr.random_depth(rng, 3, H, W)
    mask = np.zeros((3, H, W, 3), np.uint8)
    mask[0] = np.repeat(rng.choice(np.array([239, 240, 241, 242], np.uint8), (H, W, 1)), 3, axis=2)      # grey 240 is out, 241 is in
    mask[1] = rng.integers(225, 256, (H, W, 3), dtype=np.uint8)                                        # coloured, on either side of 240
    mask[2, ::2] = [255, 255, 0]                                                                       # yellow: gray 226
    mask[2, 1::4] = [255, 242, 200]                                                                    # gray 241 ...
    mask[2, 3::4] = [200, 242, 255]                                                                    # ... and 231 with R and B swapped
    g = cr.gray_of(mask)
    assert np.array_equal(g[0], mask[0, ..., 0])                                                       # the identity on R = G = B
    assert (g[1] == 240).any() and (g[1] == 241).any() and (g[1] > 241).any() and (g[1] < 240).any()
    assert (g[2, 0, 0], g[2, 1, 0], g[2, 3, 0]) == (226, 241, 231)
    want, n = cr.clip_means(depth, mask)
    assert n[0] == int((mask[0, ..., 0] >= 241).sum())
    for bgr in (False, True):
        d = torch.from_numpy(np.ascontiguousarray(depth[..., ::-1]) if bgr else depth).cuda()
        m = torch.from_numpy(np.ascontiguousarray(mask[..., ::-1]) if bgr else mask).cuda()
        means, counts = fcd.convergence_depths(d, m, bgr=bgr, counts=True)
        _check(means.cpu().numpy(), want, f"threshold bgr={bgr}")
        assert counts.cpu().numpy().tolist() == n.tolist()


def _raw(_lib, ctx, depth, mask, n_mask, means, counts=None, *, W=None, H=None, n_frames=None, max_depth=100.0, depth_order=0,
         mask_order=0, depth_pitch=None, depth_stride=None, mask_pitch=None, mask_stride=None, stream=None, null_depth=False,
         null_means=False):
    N, h, w = (int(v) for v in depth.shape[:3])
    return _lib.load().mdvt_convergence_depths(
        ctx.handle, w if W is None else W, h if H is None else H,
        None if null_depth else depth.data_ptr(), depth.stride(1) if depth_pitch is None else depth_pitch,
        depth.stride(0) if depth_stride is None else depth_stride, depth_order,
        mask.data_ptr() if mask is not None else None, (mask.stride(1) if mask is not None else 0) if mask_pitch is None else mask_pitch,
        (mask.stride(0) if mask is not None else 0) if mask_stride is None else mask_stride, mask_order,
        N if n_frames is None else n_frames, n_mask, float(max_depth), None if null_means else means.data_ptr(),
        counts.data_ptr() if counts is not None else None, C.c_void_p(stream.cuda_stream) if stream is not None else None)


def _batch(rng, N, n_mask, H, W, empty=None):
    depth = cr.random_depth(rng, N, H, W)
    mask = np.repeat(rng.choice(np.array([0, 255], np.uint8), (n_mask, H, W, 1), p=(0.7, 0.3)), 3, axis=3)
    if empty is not None:
        mask[empty] = 17
    return depth, mask


def test_a_batch_with_a_short_mask_on_two_streams(mods):
    torch, _lib, fcd = mods
    W, H = 205, 83
    depth, mask = _batch(np.random.default_rng(5), 5, 3, H, W, empty=1)
    want, n = cr.clip_means(depth, mask)
    assert n[1] == 0 and n[3] == n[4] == W * H and np.isnan(want[1])
    d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda()
    means, counts = fcd.convergence_depths(d, m, counts=True)
    _check(means.cpu().numpy(), want, "batch of 5, 3 mask frames")
    assert counts.cpu().numpy().tolist() == n.tolist()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    means2 = fcd.convergence_depths(d, m, stream=side)
    side.synchronize()
    _check(means2.cpu().numpy(), want, "batch of 5 on a side stream")
    torch.cuda.current_stream().wait_stream(side)


def test_a_batch_larger_than_one_launch_set(mods):
    """workspace_mib = 1: a masked 171 x 96 frame takes about 35 KiB of workspace, so 40 frames run in two launch sets; the mask
    runs out inside the second."""
    torch, _lib, fcd = mods
    W, H, N, M = 171, 96, 40, 33
    depth, mask = _batch(np.random.default_rng(40), N, M, H, W, empty=30)
    want, n = cr.clip_means(depth, mask)
    ctx = _lib.Context(0, 16, 16)
    try:
        cfg = _lib.MdvtConfig(mode=_lib.MODE_POINTS, ipd_m=0.063, max_depth=100.0, workspace_mib=1)
        ctx.check(_lib.load().mdvt_set_config(ctx.handle, C.byref(cfg)))
        d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda()
        means = torch.full((N,), -1.0, dtype=torch.float32, device="cuda")
        counts = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        ctx.check(_raw(_lib, ctx, d, m, M, means, counts))
        torch.cuda.synchronize()
        _check(means.cpu().numpy(), want, "40 frames in launch sets")
        assert counts.cpu().numpy().tolist() == n.tolist()
        assert ctx.workspace_bytes() <= 1 << 20
    finally:
        ctx.close()


def test_every_refusal_leaves_the_means_untouched(mods):
    torch, _lib, fcd = mods
    W, H, N = 20, 6, 3
    depth, mask = _batch(np.random.default_rng(6), N, N, H, W)
    d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda()
    means = torch.full((N,), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    ctx = _lib.Context(0, 16, 16)
    try:
        cases = [
            ("NULL d_depth", dict(null_depth=True), INVALID),
            ("NULL d_means", dict(null_means=True), INVALID),
            ("depth pitch below 3 * width", dict(depth_pitch=3 * W - 1), INVALID),
            ("mask pitch below 3 * width", dict(mask_pitch=3 * W - 1), INVALID),
            ("depth stride below height * pitch", dict(depth_stride=H * 3 * W - 1), INVALID),
            ("mask stride below height * pitch", dict(mask_stride=H * 3 * W - 1), INVALID),
            ("n_frames 0", dict(n_frames=0, n_mask=0), INVALID),
            ("n_frames negative", dict(n_frames=-1, n_mask=0), INVALID),
            ("n_mask_frames negative", dict(n_mask=-1), INVALID),
            ("n_mask_frames above n_frames", dict(n_mask=N + 1), INVALID),
            ("mask frames without a mask", dict(no_mask=True, n_mask=1), INVALID),
            ("max_depth 0", dict(max_depth=0.0), INVALID),
            ("max_depth negative", dict(max_depth=-100.0), INVALID),
            ("max_depth NaN", dict(max_depth=float("nan")), INVALID),
            ("unknown depth order", dict(depth_order=2), INVALID),
            ("unknown mask order", dict(mask_order=-1), INVALID),
            ("width * height above 2^28", dict(W=32768, H=8193, n_frames=1, n_mask=0, depth_pitch=3 * 32768), UNSUPPORTED),
        ]
        for what, kw, status in cases:
            kw = dict(kw)
            n_mask = kw.pop("n_mask", N)
            rc = _raw(_lib, ctx, d, None if kw.pop("no_mask", False) else m, n_mask, means, counts, **kw)
            torch.cuda.synchronize()
            assert rc == status, f"{what}: status {rc}"
            assert (means.cpu().numpy() == -7.0).all() and (counts.cpu().numpy() == -7).all(), f"{what}: a refused call wrote"
            assert _lib.load().mdvt_last_error(ctx.handle), what
        ctx.check(_raw(_lib, ctx, d, m, N, means, counts))                                  # the same buffers, accepted
        torch.cuda.synchronize()
        want, n = cr.clip_means(depth, mask)
        _check(means.cpu().numpy(), want, "after the refusals")
        assert counts.cpu().numpy().tolist() == n.tolist()
    finally:
        ctx.close()
