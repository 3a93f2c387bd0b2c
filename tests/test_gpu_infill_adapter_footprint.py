"""The four entry points of include/mdvt_infill_adapter.h held to their footprints with the arenas of tests/footprint.py, through the
raw C ABI: nothing outside the stated footprint changes; every byte inside it is written (each case runs on a poison and on its
complement); a refused call leaves everything as it was; one case has its frames more than 4 GiB apart.  The arenas of the
side-by-side frames hold ONE eye's half of each row -- the other half is the arena's pitch padding (and, for the right eye, the
guard in front of it) -- so "depends on no byte outside the eye's half" and "writes only the eye's half" are checked like every
other padding.  Expected values: tests/infill_adapter_ref.py, bit for bit.  (The entry points are declared outside include/mdvt.h,
so their case families live here; their tally rows are printed here and taken out of the shared table again.)"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import infill_adapter_ref as R

pytestmark = pytest.mark.gpu

PREPARE, MOMENTS, APPLY, COMPOSITE = "mdvt_adapter_prepare_eye", "mdvt_lhm_moments", "mdvt_lhm_apply", "mdvt_adapter_composite_eye"
INVALID = -1


def _vp(a, back=0):
    return C.c_void_p(a.ptr - back)


@pytest.fixture(autouse=True)
def torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        for e in (PREPARE, MOMENTS, APPLY, COMPOSITE):
            fp.TALLY.pop(e, None)


@pytest.fixture()
def lib():
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    yield _lib.load(), ctx
    ctx.close()


def half(lay, ew):
    """The layout of an arena that holds one eye's half of side-by-side rows: the other half is padding."""
    return fp.Layout(lay.base, lay.pad + 3 * ew, lay.gap)


def aligned(lay, unit):
    return fp.Layout(lay.base - lay.base % unit, 0, 0)


def _prepare_case(L, ctx, rng, n, ew, eh, mw, mh, eye, lays, kind):
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, kind)
    want = R.prepare_eye(color, mask, eye, mw, mh)
    lc, lm, li, lk, lh = half(lays.u8(), ew), half(lays.u8(), ew), lays.u8(), lays.u8(), aligned(lays.u8(), 4)
    back = eye * 3 * ew

    def body(run, short=False):
        ac = run.inp("color", R.eye_of(color, eye), lc)
        am = run.inp("mask", R.eye_of(mask, eye), lm)
        ai, ak = run.out("image", mh, 3 * mw, n, li), run.out("model_mask", mh, mw, n, lk)
        ah = run.out("holes", 1, 4 * n, 1, lh)
        rc = L.mdvt_adapter_prepare_eye(ctx.handle, ew, eh, n, eye, _vp(ac, back), ac.pitch, ac.stride, _vp(am, back), am.pitch, am.stride, mw, mh,
                                        _vp(ai), 3 * mw - 1 if short else ai.pitch, ai.stride, _vp(ak), ak.pitch, ak.stride, _vp(ah), None)
        if not short:
            ctx.check(rc)
        return rc
    return body, want, f"prepare eye {eye} {n}x{ew}x{eh} -> {mw}x{mh} {kind} {lc} {lm} {li} {lk}"


SIZES = [((9, 8), (16, 12)), ((16, 12), (7, 5)), ((16, 12), (8, 6)), ((13, 9), (13, 9)), ((33, 17), (24, 11))]


def test_prepare_eye_footprint(own_tally, lib):
    L, ctx = lib
    for k, (rng, lays) in enumerate(fp.layout_sweep(4, 1510)):
        (ew, eh), (mw, mh) = SIZES[k % len(SIZES)]
        n, eye = 1 + k % 3, k % 2
        body, (wi, wm, wc), tag = _prepare_case(L, ctx, rng, n, ew, eh, mw, mh, eye, lays, ("mixed", "all", "none", "border")[k % 4])
        out = fp.twice(PREPARE, body, seed=k, what=tag)
        fp.accepted(PREPARE)
        assert np.array_equal(out["image"].reshape(n, mh, mw, 3), wi), tag
        assert np.array_equal(out["model_mask"].reshape(n, mh, mw), wm), tag
        assert np.array_equal(np.ascontiguousarray(out["holes"]).view(np.uint32).reshape(n), wc), tag
        if k % 4 == 0:
            fp.refused(PREPARE, lambda run: body(run, short=True), INVALID, seed=k)
    fp.finish_entry(PREPARE, need_odd=True, need_padded=True)
    t = fp.tally(PREPARE)
    assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]


def _moments_case(L, ctx, rng, n, H, W, lays, k):
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    with_mask = k % 3 != 1
    mask = ((rng.random((n, H, W)) < 0.4) * rng.integers(1, 256, (n, H, W))).astype(np.uint8)
    want = R.moments(frames, mask if with_mask else None)
    lf, lm, lo = lays.u8(), lays.u8(), aligned(lays.u8(), 8)

    def body(run, short=False):
        af, am = run.inp("frames", frames, lf), run.inp("mask", mask, lm)
        ao = run.out("moments", 1, 80 * n, 1, lo)
        rc = L.mdvt_lhm_moments(ctx.handle, W, H, n, _vp(af), 3 * W - 1 if short else af.pitch, af.stride, _vp(am) if with_mask else None, am.pitch, am.stride,
                                _vp(ao), None)
        if not short:
            ctx.check(rc)
        run.vector = fp.all_aligned([af] + ([am] if with_mask else []), 4)
        return rc
    return body, want, f"moments {n}x{W}x{H} mask={with_mask} {lf} {lm}"


def test_lhm_moments_footprint(own_tally, lib):
    L, ctx = lib
    vector = 0
    for k, (rng, lays) in enumerate(fp.layout_sweep(4, 1511)):
        W, H = int(rng.choice(fp.WIDTHS)), int(rng.choice(fp.HEIGHTS))
        if lays.vec:
            W = max(8, W & ~3)
        n = 1 + k % 3
        body, want, tag = _moments_case(L, ctx, rng, n, H, W, lays, k)
        box = {}

        def accepted_body(run):
            body(run)
            box["vector"] = run.vector
        out = fp.twice(MOMENTS, accepted_body, seed=k, what=tag)
        fp.accepted(MOMENTS, vector=box["vector"])
        vector += int(box["vector"])
        got = np.ascontiguousarray(out["moments"]).view(np.uint64).reshape(n, 10)
        assert [[int(v) for v in row] for row in got] == want, tag
        if k % 4 == 0:
            fp.refused(MOMENTS, lambda run: body(run, short=True), INVALID, seed=k)
    fp.finish_entry(MOMENTS, need_odd=True, need_padded=True)
    assert vector >= 2, "no layout reached the dword loads"
    t = fp.tally(MOMENTS)
    assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]


def _apply_case(L, ctx, rng, n, H, W, lays, k):
    video = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    reference = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8) // (1 + k % 3) + 10 * (k % 5)
    reference = reference.astype(np.uint8)
    mx, mr = R.moments(video), R.moments(reference)
    params = np.array([R.lhm_params(mx[i], mr[i], mr[i]) for i in range(n)])
    want = np.array([R.lhm_apply(video[i], params[i])[0] for i in range(n)])
    li, lo, lp = lays.u8(), lays.u8(), aligned(lays.u8(), 8)

    def body(run, short=False):
        ai = run.inp("video", video, li)
        ap = run.inp("params", params.reshape(1, 1, -1), lp)
        ao = run.out("out", H, 3 * W, n, lo)
        rc = L.mdvt_lhm_apply(ctx.handle, W, H, n, _vp(ai), ai.pitch, ai.stride, _vp(ap), _vp(ao), 3 * W - 1 if short else ao.pitch, ao.stride, None)
        if not short:
            ctx.check(rc)
        run.vector = fp.all_aligned([ai, ao], 4) and W >= 4
        return rc
    return body, want, f"apply {n}x{W}x{H} {li} {lo}"


def test_lhm_apply_footprint(own_tally, lib):
    L, ctx = lib
    vector = 0
    for k, (rng, lays) in enumerate(fp.layout_sweep(4, 1512)):
        W, H = int(rng.choice(fp.WIDTHS)), int(rng.choice(fp.HEIGHTS))
        if lays.vec:
            W = max(8, W & ~3)
        n = 1 + k % 3
        body, want, tag = _apply_case(L, ctx, rng, n, H, W, lays, k)
        box = {}

        def accepted_body(run):
            body(run)
            box["vector"] = run.vector
        out = fp.twice(APPLY, accepted_body, seed=k, what=tag)
        fp.accepted(APPLY, vector=box["vector"])
        vector += int(box["vector"])
        assert np.array_equal(out["out"].reshape(n, H, W, 3), want), tag
        if k % 4 == 0:
            fp.refused(APPLY, lambda run: body(run, short=True), INVALID, seed=k)
    fp.finish_entry(APPLY, need_odd=True, need_padded=True, need_vector=True)
    assert vector >= 2, "no layout reached the dword path"
    t = fp.tally(APPLY)
    assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]


def _composite_case(L, ctx, rng, orc, n, ew, eh, mw, mh, eye, lays, kind):
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, kind)
    model = rng.integers(0, 256, (n, mh, mw, 3), dtype=np.uint8)
    want = R.composite_eye(model, color, mask, eye, orc)
    lc, lm, lf, lp, lb = half(lays.u8(), ew), half(lays.u8(), ew), lays.u8(), half(lays.u8(), ew), half(lays.u8(), ew)
    back = eye * 3 * ew

    def body(run, short=False):
        ac, am = run.inp("color", R.eye_of(color, eye), lc), run.inp("mask", R.eye_of(mask, eye), lm)
        af = run.inp("model", model, lf)
        ap, ab = run.out("pasted", eh, 3 * ew, n, lp), run.out("blended", eh, 3 * ew, n, lb)
        rc = L.mdvt_adapter_composite_eye(ctx.handle, ew, eh, n, eye, _vp(af), mw, mh, af.pitch, af.stride, _vp(ac, back), ac.pitch, ac.stride,
                                          _vp(am, back), am.pitch, am.stride, _vp(ap, back), ap.pitch, ap.stride,
                                          _vp(ab, back), 6 * ew - 1 if short else ab.pitch, ab.stride, None)
        if not short:
            ctx.check(rc)
        return rc
    return body, want, f"composite eye {eye} {n}x{ew}x{eh} <- {mw}x{mh} {kind} {lc} {lm} {lf} {lp} {lb}"


def test_composite_eye_footprint(own_tally, lib, orc):
    L, ctx = lib
    for k, (rng, lays) in enumerate(fp.layout_sweep(4, 1513)):
        (mw, mh), (ew, eh) = SIZES[k % len(SIZES)]
        ew, eh = max(ew, 8), max(eh, 8)
        n, eye = 1 + k % 3, k % 2
        body, (wp, wb), tag = _composite_case(L, ctx, rng, orc, n, ew, eh, mw, mh, eye, lays, ("mixed", "all", "none", "border")[k % 4])
        out = fp.twice(COMPOSITE, body, seed=k, what=tag)
        fp.accepted(COMPOSITE)
        assert np.array_equal(out["pasted"].reshape(n, eh, ew, 3), wp), tag
        assert np.array_equal(out["blended"].reshape(n, eh, ew, 3), wb), tag
        if k % 4 == 0:
            fp.refused(COMPOSITE, lambda run: body(run, short=True), INVALID, seed=k)
    fp.finish_entry(COMPOSITE, need_odd=True, need_padded=True)
    t = fp.tally(COMPOSITE)
    assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]


@pytest.fixture(scope="module")
def slab():
    """One sparse slab for the far case.  The one permitted skip: less than twice the slab free on the device."""
    import torch
    reason = fp.Slab.skip_reason()
    if reason:
        pytest.skip(reason)
    s = fp.Slab()
    yield s
    del s.buf
    torch.cuda.empty_cache()


FAR_STRIDE = 1 << 32                                   # two frames: the second more than 4 GiB behind the first


def test_prepare_moments_and_apply_with_frames_more_than_4_gib_apart(slab, lib):
    L, ctx = lib
    rng = np.random.default_rng(1520)
    cases = [(PREPARE, _prepare_case(L, ctx, rng, 2, 16, 12, 7, 5, 0, fp.Layouts(rng, (1, 3, 1)), "mixed"), 4),
             (MOMENTS, _moments_case(L, ctx, rng, 2, 9, 36, fp.Layouts(rng, (4, 4, 4), vec=True), 0), 2),
             (APPLY, _apply_case(L, ctx, rng, 2, 9, 37, fp.Layouts(rng, (1, 3, 1)), 0), 2)]
    for entry, (body, want, tag), n_far in cases:
        def far_body(run):
            body(run)
            far = [a for a in run.arenas.values() if a.n_frames > 1]
            assert len(far) == n_far and all(a.stride > 1 << 32 for a in far), tag
        try:
            with fp.far(fp.Far(slab, "stride", stride_unit=FAR_STRIDE)):
                out = fp.twice(entry, far_body, seed=7, what=tag + " [far stride]")
        finally:
            fp.TALLY.pop(entry, None)
        if entry == PREPARE:
            assert np.array_equal(out["image"].reshape(want[0].shape), want[0]) and np.array_equal(out["model_mask"].reshape(want[1].shape), want[1])
            assert np.array_equal(np.ascontiguousarray(out["holes"]).view(np.uint32).reshape(2), want[2])
        elif entry == MOMENTS:
            got = np.ascontiguousarray(out["moments"]).view(np.uint64).reshape(2, 10)
            assert [[int(v) for v in row] for row in got] == want
        else:
            assert np.array_equal(out["out"].reshape(want.shape), want)
