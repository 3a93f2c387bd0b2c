"""mdvt_scale_shift_fit and mdvt_metric_depth_codes (include/mdvt_metric_align.h) and their Python faces in video_metric_convert
against NumPy on the test machine (tests/metric_align_ref.py): the fit's 8 floats, the code bytes and the coded depth planes bit for
bit -- the same 32 bits, or both NaN; no tolerance -- at every size where the order of summation can go wrong, on padded and odd layouts, on the
16-byte load path and the element path, with every value set the reference can meet, on streams, across launch sets, and every refusal.

Which layouts take the 16-byte loads (the library does not report it; include/mdvt_metric_align.h states it): a plane whose address,
pitch and stride are multiples of 16 bytes with a width that is a multiple of 4, or a plane without any padding at an address that is a
multiple of 16 (any width).  The tests below name the path each layout takes by that rule."""
import ctypes as C

import numpy as np
import pytest

import metric_align_ref as mr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
F = np.float32


@pytest.fixture(scope="module")
def mods():
    import torch
    from metric_depth_video_toolbox_amd import _lib, video_metric_convert as vmc
    return torch, _lib, vmc


def _strided(torch, planes, pad, gap, base):
    """The planes inside a poisoned buffer (NaN, or 0xFF bytes): rows pad and frames gap values longer, `base` values in."""
    planes = np.ascontiguousarray(planes)
    N, H, W = planes.shape
    pitch = W + pad
    stride = H * pitch + gap
    t = torch.from_numpy(planes.view(np.uint8) if planes.dtype == bool else planes).cuda()
    buf = torch.full((base + N * stride + 64,), float("nan") if t.dtype == torch.float32 else 0xFF, dtype=t.dtype, device="cuda")
    view = torch.as_strided(buf, (N, H, W), (stride, pitch, 1), base)
    view.copy_(t)
    return view.view(torch.bool) if planes.dtype == bool else view


def _check8(got, want, what):
    got = np.asarray(got, F)
    bad = mr.same_bits(got, want)
    print(f"{what}: {len(bad)} of 8 floats differ; scale {want[5]!r} shift {want[6]!r}")
    names = "a_00 a_01 a_11 b_0 b_1 scale shift det".split()
    assert bad.size == 0, f"{what}: " + ", ".join(f"{names[i]} got {got[i]!r} ({got[i].tobytes().hex()}) want {want[i]!r} ({want[i].tobytes().hex()})"
                                                   for i in bad)


# Every fit input is drawn by metric_align_ref.fit_input from a (generator, shape, seed) listed in metric_align_ref.FIT_INPUTS, where
# tests/test_metric_align_cpu.py holds those very arrays to the condition that they tell the orders of summation apart.
def _ids(cases):
    return ["x".join(map(str, shape)) for _, shape, _ in cases]


@pytest.mark.parametrize("case", mr.FIT_INPUTS["every_size"], ids=_ids(mr.FIT_INPUTS["every_size"]))
def test_fit_equals_numpy_at_every_size(mods, case):
    """Dense planes (16-byte loads) and the same data with padded pitches, strides with gaps and bases at odd float offsets (element
    by element): a chunk boundary and a leaf boundary fall mid-row and between frames at (3, 37, 53), (5, 41, 83), (32, 98, 174)."""
    torch, _lib, vmc = mods
    shape = case[1]
    p, d, m = mr.fit_input(*case)
    t = mr.inverse(d)
    for mask in (None, m):
        want = mr.fit(mr.concat(p), mr.concat(t), None if mask is None else mr.concat(mask))
        got = vmc.compute_scale_and_shift_full(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda(),
                                               None if mask is None else torch.from_numpy(mask).cuda())
        _check8(got.numpy(), want, f"{shape} dense mask={mask is not None}")
        got = vmc.compute_scale_and_shift_full(_strided(torch, p, 3, 5, 1), _strided(torch, t, 1, 7, 3),
                                               None if mask is None else _strided(torch, mask, 5, 3, 1))
        _check8(got.numpy(), want, f"{shape} padded mask={mask is not None}")
    s, h = got.scale_shift()
    assert isinstance(s, np.float32) and s.tobytes() == want[5].tobytes() and h.tobytes() == want[6].tobytes()


@pytest.mark.parametrize("case", mr.FIT_INPUTS["vector"], ids=_ids(mr.FIT_INPUTS["vector"]))
def test_fit_vector_and_element_paths_give_the_same_bits(mods, case):
    """Widths that are multiples of 4: rows padded by 4 and 8 floats, frame gaps of 16, bases 4 floats in (16-byte loads, mask 4-byte
    loads, with padding) against the same data 1 float in (element by element) and against NumPy."""
    torch, _lib, vmc = mods
    shape = case[1]
    p, d, m = mr.fit_input(*case)
    t = mr.inverse(d)
    want = mr.fit(mr.concat(p), mr.concat(t), mr.concat(m))
    vec = [_strided(torch, p, 4, 16, 4), _strided(torch, t, 8, 0, 8), _strided(torch, m, 4, 16, 4)]
    assert all(v.data_ptr() % (16 if v.dtype == torch.float32 else 4) == 0 for v in vec)
    one = vmc.compute_scale_and_shift_full(*vec).numpy()
    _check8(one, want, f"{shape} 16-byte loads")
    odd = [_strided(torch, p, 4, 16, 1), _strided(torch, t, 8, 0, 3), _strided(torch, m, 4, 16, 1)]
    assert all(v.data_ptr() % 16 != 0 for v in odd[:2])
    two = vmc.compute_scale_and_shift_full(*odd).numpy()
    _check8(two, want, f"{shape} element by element")
    assert one.tobytes() == two.tobytes()


def test_fit_value_sets(mods):
    torch, _lib, vmc = mods
    spread, with_zero, no_prediction, masked = mr.FIT_INPUTS["value_sets"]
    shape = spread[1]
    rng = np.random.default_rng(53)                                 # (the bool mask only)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # magnitudes over 1e-3 ... 1e3
    p, d, _ = mr.fit_input(*spread)
    want = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)))
    _check8(vmc.compute_scale_and_shift_full(cuda(p), cuda(mr.inverse(d))).numpy(), want, "spread")
    # the library's own inverse
    _check8(vmc.compute_scale_and_shift_full(cuda(p), cuda(d), target_is_depth=True).numpy(), want, "spread, target_is_depth")
    _check8(vmc.compute_scale_and_shift_full(_strided(torch, p, 3, 5, 1), _strided(torch, d, 1, 0, 1), target_is_depth=True).numpy(), want,
            "spread, target_is_depth, padded")
    # a depth of 0: the target holds inf, the sums inf and NaN in NumPy's order
    p, d, m = mr.fit_input(*with_zero)
    d[0, 5, 7] = 0
    d[2, 36, 52] = 0
    for mask in (None, m):
        want = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)), None if mask is None else mr.concat(mask))
        assert not np.isfinite(want[3]) and np.isnan(want[5])
        _check8(vmc.compute_scale_and_shift_full(cuda(p), cuda(d), None if mask is None else cuda(mask), target_is_depth=True).numpy(), want,
                f"depth 0, mask={mask is not None}")
    # ... and masked away where the mask byte is 0 only if 0 * inf were 0: it is NaN, as in the reference
    mask = np.ones(shape, np.uint8)
    mask[0, 5, 7] = mask[2, 36, 52] = 0
    want = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)), mr.concat(mask))
    assert np.isnan(want[4])
    _check8(vmc.compute_scale_and_shift_full(cuda(p), cuda(mr.inverse(d)), cuda(mask)).numpy(), want, "depth 0 under a mask of 0")
    # det == 0: one element; all predictions 0
    one = vmc.compute_scale_and_shift_full(cuda(np.array([[2.5]], F)), cuda(np.array([[0.25]], F))).numpy()
    _check8(one, mr.fit(np.array([[2.5]], F), np.array([[0.25]], F)), "one element")
    assert (one[5], one[6], one[7]) == (1, 0, 0)
    p0, d = np.zeros(shape, F), mr.fit_input(*no_prediction)[1]
    zero = vmc.compute_scale_and_shift_full(cuda(p0), cuda(mr.inverse(d))).numpy()
    _check8(zero, mr.fit(mr.concat(p0), mr.concat(mr.inverse(d))), "all predictions 0")
    assert (zero[5], zero[6], zero[7]) == (1, 0, 0)
    # masks: bool, uint8 with 0, 1 and 3, all zero
    p, d, m3 = mr.fit_input(*masked)
    t = mr.inverse(d)
    mb = rng.random(shape) < 0.6
    for name, m in (("uint8 0/1/3", m3), ("bool", mb), ("all zero", np.zeros(shape, np.uint8))):
        want = mr.fit(mr.concat(p), mr.concat(t), mr.concat(m))
        _check8(vmc.compute_scale_and_shift_full(cuda(p), cuda(t), cuda(m)).numpy(), want, f"mask {name}")
        _check8(vmc.compute_scale_and_shift_full(_strided(torch, p, 1, 1, 1), cuda(t), _strided(torch, m, 3, 1, 3)).numpy(), want, f"mask {name}, padded")
    assert (want[5], want[6], want[7]) == (1, 0, 0)                 # the all-zero mask: every sum is 0
    # [H, W] inputs
    want = mr.fit(p[0], t[0], m3[0])
    _check8(vmc.compute_scale_and_shift_full(cuda(p[0]), cuda(t[0]), cuda(m3[0])).numpy(), want, "one [H, W] plane")


def test_fit_on_a_side_stream(mods):
    torch, _lib, vmc = mods
    p, d, _ = mr.fit_input(*mr.FIT_INPUTS["side_stream"][0])
    want = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)))
    dp, dd = torch.from_numpy(p).cuda(), torch.from_numpy(d).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = vmc.compute_scale_and_shift_full(dp, dd, target_is_depth=True, stream=side)
    side.synchronize()
    _check8(got.numpy(), want, "side stream")
    torch.cuda.current_stream().wait_stream(side)


def _raw_fit(_lib, ctx, p, t, m, out, *, W=None, H=None, N=None, tid=0, null=(), p_pitch=None, p_stride=None, t_pitch=None, t_stride=None,
             m_pitch=None, m_stride=None, stream=None):
    n, h, w = (int(v) for v in p.shape)
    ptr = lambda name, x: None if name in null or x is None else x.data_ptr()
    return _lib.load().mdvt_scale_shift_fit(
        ctx.handle, w if W is None else W, h if H is None else H, n if N is None else N,
        ptr("pred", p), 4 * p.stride(1) if p_pitch is None else p_pitch, 4 * p.stride(0) if p_stride is None else p_stride,
        ptr("target", t), 4 * t.stride(1) if t_pitch is None else t_pitch, 4 * t.stride(0) if t_stride is None else t_stride, tid,
        ptr("mask", m), (m.stride(1) if m is not None else 0) if m_pitch is None else m_pitch,
        (m.stride(0) if m is not None else 0) if m_stride is None else m_stride, ptr("out", out),
        C.c_void_p(stream.cuda_stream) if stream is not None else None)


def test_fits_of_growing_sizes_on_one_context_and_more_than_one_launch_set(mods):
    """A fresh context: a small fit, a larger one (the scratch block grows), the small one again, then 1026 chunks -- more than the
    1024 of one launch set, so the totals travel between two sets -- and the small one once more."""
    torch, _lib, vmc = mods
    ctx = _lib.Context(0, 16, 16)
    try:
        cases = {}
        for case in mr.FIT_INPUTS["growth"]:
            shape = case[1]
            p, d, _ = mr.fit_input(*case)
            cases[shape] = (torch.from_numpy(p).cuda(), torch.from_numpy(d).cuda(), mr.fit(mr.concat(p), mr.concat(mr.inverse(d))))
        assert (2 * 2053 * 2047 + 8191) // 8192 == 1026
        out = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
        grown = []
        for shape in ((1, 3, 43), (5, 41, 83), (1, 3, 43), (2, 2053, 2047), (1, 3, 43)):
            p, d, want = cases[shape]
            ctx.check(_raw_fit(_lib, ctx, p, d, None, out, tid=1))
            torch.cuda.synchronize()
            _check8(out.cpu().numpy(), want, f"{shape} on one context")
            grown.append(ctx.workspace_bytes())
        assert grown[0] <= grown[1] == grown[2] < grown[3] == grown[4] <= 1 << 20, grown       # (the pool hands out size classes)
    finally:
        ctx.close()


def test_every_fit_refusal_leaves_the_output_untouched(mods):
    torch, _lib, vmc = mods
    N, H, W = mr.FIT_INPUTS["refusals"][0][1]
    p, d, m = mr.fit_input(*mr.FIT_INPUTS["refusals"][0])
    dp, dt, dm = torch.from_numpy(p).cuda(), torch.from_numpy(mr.inverse(d)).cuda(), torch.from_numpy(m).cuda()
    out = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
    ctx = _lib.Context(0, 16, 16)
    try:
        cases = [
            ("NULL d_pred", dict(null=("pred",)), INVALID),
            ("NULL d_target", dict(null=("target",)), INVALID),
            ("NULL d_out", dict(null=("out",)), INVALID),
            ("prediction pitch below 4 * width", dict(p_pitch=4 * W - 1), INVALID),
            ("target pitch below 4 * width", dict(t_pitch=4 * W - 4), INVALID),
            ("mask pitch below width", dict(m_pitch=W - 1), INVALID),
            ("prediction stride below height * pitch", dict(p_stride=4 * W * H - 4), INVALID),
            ("target stride below height * pitch", dict(t_stride=4 * W * H - 1), INVALID),
            ("mask stride below height * pitch", dict(m_stride=W * H - 1), INVALID),
            ("n_frames 0", dict(N=0), INVALID),
            ("n_frames negative", dict(N=-2), INVALID),
            ("width 0", dict(W=0), INVALID),
            ("height negative", dict(H=-1), INVALID),
            ("target_is_depth 2", dict(tid=2), INVALID),
            ("2^31 values", dict(N=2, W=32768, H=32768, p_pitch=4 * 32768, t_pitch=4 * 32768, m_pitch=32768, p_stride=1 << 32, t_stride=1 << 32,
                                 m_stride=1 << 30), UNSUPPORTED),
        ]
        for what, kw, status in cases:
            rc = _raw_fit(_lib, ctx, dp, dt, dm, out, **kw)
            torch.cuda.synchronize()
            assert rc == status, f"{what}: status {rc}"
            assert (out.cpu().numpy() == -7.0).all(), f"{what}: a refused call wrote"
            assert _lib.load().mdvt_last_error(ctx.handle), what
        assert _lib.load().mdvt_scale_shift_fit(None, W, H, N, dp.data_ptr(), 4 * W, 4 * W * H, dt.data_ptr(), 4 * W, 4 * W * H, 0, None, 0, 0,
                                                out.data_ptr(), None) == INVALID
        ctx.check(_raw_fit(_lib, ctx, dp, dt, dm, out))             # the same buffers, accepted
        torch.cuda.synchronize()
        _check8(out.cpu().numpy(), mr.fit(mr.concat(p), mr.concat(mr.inverse(d)), mr.concat(m)), "after the refusals")
    finally:
        ctx.close()


# ---- the codes ------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 5e-39, -2.0, -1e-3, 1e-3, 1e3, 1e-2, np.inf, -np.inf, 3e38, 1.5e-38], F)

# (in_w, in_h) -> (out_w, out_h); None: the same size
CASES = [((5, 3), None), ((33, 17), None), ((130, 70), None), ((33, 17), (64, 48)), ((64, 48), (33, 17)), ((17, 9), (17, 31)),
         ((1, 1), (4, 3)), ((9, 1), (3, 5)), ((132, 74), (480, 270))]


def _relative(rng, N, h, w, specials):
    x = (rng.random((N, h, w), dtype=F) * F(3)).astype(F)
    x[rng.random((N, h, w)) < 0.05] *= F(1e-3)                      # far points: depths beyond max_depth
    if specials is not None:
        flat = x.reshape(-1)
        at = rng.choice(flat.size, min(flat.size, len(specials)), replace=False)
        flat[at] = specials[:len(at)]
    return x


def _check_codes(got_codes, got_depth, want_codes, want_depth, what):
    gc = got_codes.cpu().numpy()
    bad = np.argwhere(gc != want_codes)
    msg = f"{what}: {len(bad)} code bytes of {want_codes.size} differ"
    if got_depth is not None:
        gd = got_depth.cpu().numpy()
        badd = mr.same_bits(gd, want_depth)
        msg += f", {len(badd)} depth values of {want_depth.size}"
        assert badd.size == 0, msg + f"; first at {np.unravel_index(badd[0], want_depth.shape)}: got {gd.ravel()[badd[0]]!r}, want {want_depth.ravel()[badd[0]]!r}"
    print(msg)
    assert bad.size == 0, msg + f"; first at {bad[0]}: got {gc[tuple(bad[0])]}, want {want_codes[tuple(bad[0])]}"


@pytest.mark.parametrize("style", [0, 1])
@pytest.mark.parametrize("size,out_size", CASES, ids=[f"{a[0]}x{a[1]}" + ("" if b is None else f"to{b[0]}x{b[1]}") for a, b in CASES])
def test_codes_and_depth_planes_equal_numpy(mods, style, size, out_size):
    """Both byte orders, 1 and 5 frames, dense and padded inputs and outputs, with and without the depth plane; scale = 1, shift = 0
    carries the special values (inv exactly 0, negative, subnormal -> inf, infinite; NaN in style 1 only; in style 0 only at the same
    size -- a resize of an infinite depth multiplies it by a zero weight, and tests put no NaN through style 0), a fitted-looking pair
    the ordinary ones."""
    torch, _lib, vmc = mods
    w, h = size
    ow, oh = size if out_size is None else out_size
    rng = np.random.default_rng(w * 1009 + h * 13 + ow + style)
    for k, (N, scale, shift, max_depth, bgr) in enumerate(((1, 1.0, 0.0, 100, False), (5, 0.3712, 0.0113, 100, True), (5, 0.5, -0.25, 20, False))):
        specials = None
        if scale == 1.0 and (style == 1 or out_size is None):
            specials = np.append(SPECIALS, F("nan")) if style == 1 else SPECIALS
        x = _relative(rng, N, h, w, specials)
        x.reshape(-1)[3::11] = F(0.4)                               # with scale 0.5, shift -0.25: a negative depth
        if scale == 0.5 and (style == 1 or out_size is None):
            x.reshape(-1)[::7] = F(0.5)                             # inv = 0.25 - 0.25: exactly 0 (style 0: an infinite depth)
        want_codes, want_depth = mr.metric_codes(x, scale, shift, max_depth, style, out_size, bgr)
        assert not np.isnan(want_depth).any()
        ss = torch.tensor([scale, shift], dtype=torch.float32, device="cuda")
        # dense, with the depth plane
        codes, depth = vmc.metric_depth_codes(torch.from_numpy(x).cuda(), ss, max_depth, style=style, out_size=out_size, bgr=bgr, want_depth=True)
        assert codes.shape == (N, oh, ow, 3) and depth.shape == (N, oh, ow)
        _check_codes(codes, depth, want_codes, want_depth, f"style {style} {size}->{out_size} set {k} dense")
        # padded input (1 float in: the element path) and padded output (odd pitch: byte stores), without the depth plane
        buf = torch.full((N * (oh * (3 * ow + 5) + 7) + 3,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(buf, (N, oh, ow, 3), (oh * (3 * ow + 5) + 7, 3 * ow + 5, 3, 1), 3)
        got = vmc.metric_depth_codes(_strided(torch, x, 3, 5, 1), ss, max_depth, style=style, out_size=out_size, bgr=bgr, out=out)
        assert got is out
        _check_codes(out, None, want_codes, None, f"style {style} {size}->{out_size} set {k} padded")
        seen = buf.cpu().numpy().copy()
        np.lib.stride_tricks.as_strided(seen[3:], (N, oh, 3 * ow), (oh * (3 * ow + 5) + 7, 3 * ow + 5, 1))[...] = 0xA5
        assert (seen == 0xA5).all(), "bytes outside the code rows changed"
        # padded, aligned output (pitch and stride multiples of 4: dword stores) with the 16-byte input path
        pitch = (3 * ow + 3) // 4 * 4 + 8
        buf = torch.full((N * (oh * pitch + 16) + 4,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.as_strided(buf, (N, oh, ow, 3), (oh * pitch + 16, pitch, 3, 1), 4)
        vmc.metric_depth_codes(_strided(torch, x, (-w) % 4 + 4, 16, 4), ss, max_depth, style=style, out_size=out_size, bgr=bgr, out=out)
        _check_codes(out, None, want_codes, None, f"style {style} {size}->{out_size} set {k} aligned and padded")
        seen = buf.cpu().numpy().copy()
        np.lib.stride_tricks.as_strided(seen[4:], (N, oh, 3 * ow), (oh * pitch + 16, pitch, 1))[...] = 0xA5
        assert (seen == 0xA5).all(), "bytes outside the code rows changed"


def test_codes_follow_a_fit_on_the_same_stream_and_agree_with_the_existing_code(mods):
    """scale and shift come from the fit's device output, on a side stream, with no host synchronisation between the calls; the codes
    are those of model_hop.depth_to_rgb_code (mdvt_encode_depth) on the returned depth planes, and decode_rgb_depth_frame of the
    codes is what the renderer sees."""
    torch, _lib, vmc = mods
    from metric_depth_video_toolbox_amd import depth_frames_helper as dfh, model_hop
    N, h, w, ow, oh = 4, 37, 53, 96, 54
    case = mr.FIT_INPUTS["codes_behind_a_fit"][0]
    assert case[1] == (N, h, w)
    p, d, _ = mr.fit_input(*case)                                   # a relative depth: affine in 1 / depth, plus noise
    want_fit = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)))
    assert np.isfinite(want_fit).all() and want_fit[5] > 0
    dp, dd = torch.from_numpy(p).cuda(), torch.from_numpy(d).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for style in (0, 1):
        fit = vmc.compute_scale_and_shift_full(dp, dd, target_is_depth=True, stream=side)
        codes, depth = vmc.metric_depth_codes(dp, fit, 100, style=style, out_size=(ow, oh), want_depth=True, stream=side)
        side.synchronize()
        _check8(fit.numpy(), want_fit, "the fit in front of the codes")
        want_codes, want_depth = mr.metric_codes(p, want_fit[5], want_fit[6], 100, style, (ow, oh))
        _check_codes(codes, depth, want_codes, want_depth, f"style {style} behind a fit")
        with torch.cuda.stream(side):
            again = model_hop.depth_to_rgb_code(depth, 100)
            seen = dfh.decode_rgb_depth_frame(codes[1].contiguous(), 100)
        side.synchronize()
        assert torch.equal(again, codes)
        u = (want_codes[1, ..., 0].astype(np.uint32) << 24) | (want_codes[1, ..., 2].astype(np.uint32) << 16)
        assert np.array_equal(seen.cpu().numpy(), u.astype(np.float32) * np.float32(100 / 255 ** 4))      # dfh:21-23
        assert np.abs(seen.cpu().numpy() - want_depth[1]).max() <= 65536 * 100 / 255 ** 4 * 1.001      # one step of the 16-bit code
    torch.cuda.current_stream().wait_stream(side)
    # convert(): the driver lines -- vda takes the first 32 frames, depthcrafter skips all-zero reference frames and lifts zeros to max_depth
    ref = d.copy()
    ref[1] = 0
    ref[2, :5] = 0
    codes = vmc.convert(dp, torch.from_numpy(ref).cuda(), 100, engine="depthcrafter", out_size=(ow, oh))
    keep = [0, 2, 3]
    lifted = np.where(ref[keep] == 0, F(100), ref[keep])
    f = mr.fit(mr.concat(p[keep]), mr.concat(mr.inverse(lifted)))
    assert np.array_equal(codes.cpu().numpy(), mr.metric_codes(p, f[5], f[6], 100, 1, (ow, oh))[0])
    codes = vmc.convert(dp, torch.from_numpy(d[:2]).cuda(), 100, engine="vda", bgr=True)
    f = mr.fit(mr.concat(p[:2]), mr.concat(mr.inverse(d[:2])))
    assert np.array_equal(codes.cpu().numpy(), mr.metric_codes(p, f[5], f[6], 100, 0, None, True)[0])


def test_every_codes_refusal_leaves_the_outputs_untouched(mods):
    torch, _lib, vmc = mods
    N, h, w, ow, oh = 2, 6, 10, 16, 9
    x = torch.rand((N, h, w), dtype=torch.float32, device="cuda")
    ss = torch.tensor([1.0, 0.5], dtype=torch.float32, device="cuda")
    codes = torch.full((N, oh, ow, 3), 0xA5, dtype=torch.uint8, device="cuda")
    depth = torch.full((N, oh, ow), -7.0, dtype=torch.float32, device="cuda")
    ctx = _lib.Context(0, 16, 16)
    L = _lib.load()

    def call(**kw):
        a = dict(in_w=w, in_h=h, n=N, rel=x.data_ptr(), rel_pitch=4 * w, rel_stride=4 * w * h, ss=ss.data_ptr(), style=0, max_depth=100.0, out_w=ow,
                 out_h=oh, codes=codes.data_ptr(), codes_pitch=3 * ow, codes_stride=3 * ow * oh, order=0, depth=depth.data_ptr(), depth_pitch=4 * ow,
                 depth_stride=4 * ow * oh)
        a.update(kw)
        return L.mdvt_metric_depth_codes(ctx.handle, a["in_w"], a["in_h"], a["n"], a["rel"], a["rel_pitch"], a["rel_stride"], a["ss"], a["style"],
                                         a["max_depth"], a["out_w"], a["out_h"], a["codes"], a["codes_pitch"], a["codes_stride"], a["order"],
                                         a["depth"], a["depth_pitch"], a["depth_stride"], None)
    try:
        cases = [
            ("NULL d_rel", dict(rel=None), INVALID), ("NULL d_scale_shift", dict(ss=None), INVALID), ("NULL d_codes", dict(codes=None), INVALID),
            ("in_w 0", dict(in_w=0), INVALID), ("in_h 0", dict(in_h=0), INVALID), ("out_w 0", dict(out_w=0), INVALID),
            ("out_h negative", dict(out_h=-1), INVALID), ("n_frames 0", dict(n=0), INVALID),
            ("rel pitch below 4 * in_w", dict(rel_pitch=4 * w - 1), INVALID), ("codes pitch below 3 * out_w", dict(codes_pitch=3 * ow - 1), INVALID),
            ("depth pitch below 4 * out_w", dict(depth_pitch=4 * ow - 4), INVALID),
            ("rel stride below a frame", dict(rel_stride=4 * w * h - 4), INVALID), ("codes stride below a frame", dict(codes_stride=3 * ow * oh - 1), INVALID),
            ("depth stride below a frame", dict(depth_stride=4 * ow * oh - 4), INVALID),
            ("style 2", dict(style=2), INVALID), ("style negative", dict(style=-1), INVALID), ("order 2", dict(order=2), INVALID),
            ("max_depth 0", dict(max_depth=0.0), INVALID), ("max_depth negative", dict(max_depth=-5.0), INVALID),
            ("max_depth NaN", dict(max_depth=float("nan")), INVALID),
            ("2^31 output pixels", dict(n=1, out_w=65536, out_h=32768, codes_pitch=3 * 65536, depth_pitch=4 * 65536), UNSUPPORTED),
        ]
        for what, kw, status in cases:
            rc = call(**kw)
            torch.cuda.synchronize()
            assert rc == status, f"{what}: status {rc}"
            assert (codes.cpu().numpy() == 0xA5).all() and (depth.cpu().numpy() == -7.0).all(), f"{what}: a refused call wrote"
            assert L.mdvt_last_error(ctx.handle), what
        ctx.check(call())
        torch.cuda.synchronize()
        want_codes, want_depth = mr.metric_codes(x.cpu().numpy(), 1.0, 0.5, 100, 0, (ow, oh))
        _check_codes(codes, depth, want_codes, want_depth, "after the refusals")
    finally:
        ctx.close()
