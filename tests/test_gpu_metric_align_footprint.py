"""mdvt_scale_shift_fit and mdvt_metric_depth_codes (include/mdvt_metric_align.h) held to their footprints with the arenas of
tests/footprint.py, through the raw C ABI: the fit writes exactly its 8 floats, the codes call the first 3 * out_w bytes of each code
row and the first 4 * out_w bytes of each depth row, nothing else; every one of those bytes is written; the results do not depend on
the bytes behind an input row's end (each case runs on a poison and on its complement); a refused call leaves everything as it was;
and one case per entry point has its frames more than 4 GiB apart.  Expected values: tests/metric_align_ref.py, bit for bit.  (The
entry points are declared outside include/mdvt.h, so their case families live here; their tally rows are printed here and taken out
of the shared table again.)"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import metric_align_ref as mr

pytestmark = pytest.mark.gpu

FIT, CODES = "mdvt_scale_shift_fit", "mdvt_metric_depth_codes"
INVALID = -1
F = np.float32


def _vp(a):
    return C.c_void_p(a.ptr)


@pytest.fixture(autouse=True)
def torch_first():
    """The arenas are torch tensors: torch opens the device before the library's context does, as in the rest of the suite."""
    import torch
    torch.cuda.init()


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop(FIT, None)                        # test_gpu_footprint.py's table lists include/mdvt.h's entry points only
        fp.TALLY.pop(CODES, None)


def _fit_case(L, ctx, rng, N, H, W, lays, k):
    """-> (body(run, short=False), want, tag) of one fit."""
    gen = mr.gen_spread if k % 2 else mr.gen_model
    p, d = gen(rng, N, H, W)
    with_mask, tid = k % 3 != 1, k % 2
    m = mr.gen_mask(rng, N, H, W)
    want = mr.fit(mr.concat(p), mr.concat(mr.inverse(d)), mr.concat(m) if with_mask else None)
    lp, lt, lm, lo = lays.w32(), lays.w32(), lays.u8(), lays.w32()

    def body(run, short=False):
        ap = run.inp("pred", p, lp)
        at = run.inp("target", d if tid else mr.inverse(d), lt)
        am = run.inp("mask", m, lm)
        ao = run.out("out", 1, 32, 1, fp.Layout(lo.base))
        rc = L.mdvt_scale_shift_fit(ctx.handle, W, H, N, _vp(ap), ap.pitch, ap.stride, _vp(at), 4 * W - 4 if short else at.pitch, at.stride, tid,
                                    _vp(am) if with_mask else None, am.pitch, am.stride, _vp(ao), None)
        if not short:
            ctx.check(rc)
        # the 16-byte loads (mask: 4-byte): address, pitch and stride multiples of 16 (4) and a width that is one of 4, or no padding at all
        def vec(a, size):
            dense = a.pitch == W * size and (N == 1 or a.stride == H * a.pitch)
            return a.ptr % (4 * size) == 0 and (dense or (W % 4 == 0 and a.pitch % (4 * size) == 0 and (N == 1 or a.stride % (4 * size) == 0)))
        run.vector = vec(ap, 4) and vec(at, 4) and (not with_mask or vec(am, 1))
        return rc
    return body, want, f"fit {N}x{H}x{W} mask={with_mask} target_is_depth={tid} {lp} {lt} {lm}"


def _codes_case(L, ctx, rng, N, h, w, ow, oh, lays, k):
    style, order, with_depth = k % 2, (k // 2) % 2, k % 3 != 2
    scale, shift, max_depth = (1.0, 0.0, 100) if k % 4 == 0 else (0.5, -0.25, 20) if k % 4 == 1 else (0.3712, 0.0113, 100)
    x = (rng.random((N, h, w), dtype=F) * F(3)).astype(F)
    if style == 1 or (w, h) == (ow, oh):
        x.reshape(-1)[::5] = np.resize(np.array([0.0, 1e-40, -2.0, 0.5, 0.4, 1e3], F), x.reshape(-1)[::5].size)
    want_codes, want_depth = mr.metric_codes(x, scale, shift, max_depth, style, (ow, oh), bool(order))
    assert not np.isnan(want_depth).any()
    lx, lc, ld, ls = lays.w32(), lays.u8(), lays.w32(), lays.w32()

    def body(run, short=False):
        ax = run.inp("rel", x, lx)
        ass = run.inp("scale_shift", np.array([[[scale, shift]]], F), fp.Layout(ls.base))
        ac = run.out("codes", oh, 3 * ow, N, lc)
        ad = run.out("depth", oh, 4 * ow, N, ld)
        rc = L.mdvt_metric_depth_codes(ctx.handle, w, h, N, _vp(ax), ax.pitch, ax.stride, _vp(ass), style, float(max_depth), ow, oh,
                                       _vp(ac), 3 * ow - 1 if short else ac.pitch, ac.stride, order, _vp(ad) if with_depth else None, ad.pitch, ad.stride, None)
        if not short:
            ctx.check(rc)
        run.vector = fp.all_aligned([ac], 4) and ow >= 4                       # the 12-byte stores of four codes
        return rc
    return body, (want_codes, want_depth), with_depth, f"codes {N}x{w}x{h}->{ow}x{oh} style={style} order={order} depth={with_depth} {lx} {lc} {ld}"


def _accept_codes(entry, body, with_depth, seed, tag):
    def body_accepted(run):
        body(run)
        if not with_depth:                             # d_depth NULL: the arena stays poison, as an input would
            run.arenas["depth"].input = run.arenas["depth"].payload(run.arenas["depth"].poison)
        body_accepted.vector = run.vector
    out = fp.twice(entry, body_accepted, seed=seed, what=tag)
    return out, body_accepted.vector


def test_scale_shift_fit_footprint(own_tally):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        vector = 0
        for k, (rng, lays) in enumerate(fp.layout_sweep(8, 1410)):
            W = int(rng.choice(fp.WIDTHS))
            H = int(rng.choice(fp.HEIGHTS + (40, 67)))     # (257 x 40, 250 x 67: more than one chunk of 8192)
            if lays.vec:
                W = max(8, W & ~3)
            N = 1 + k % 3
            body, want, tag = _fit_case(L, ctx, rng, N, H, W, lays, k)
            box = {}

            def accepted_body(run):
                body(run)
                box["vector"] = run.vector
            out = fp.twice(FIT, accepted_body, seed=k, what=tag)
            fp.accepted(FIT, vector=box["vector"])
            vector += int(box["vector"])
            got = np.ascontiguousarray(out["out"]).view(F).reshape(8)
            assert mr.same_bits(got, want).size == 0, f"{tag}: {got} vs {want}"
            if k % 4 == 0:
                fp.refused(FIT, lambda run: body(run, short=True), INVALID, seed=k)
        fp.finish_entry(FIT, need_odd=True, need_padded=True)
        assert vector >= 2, "no layout reached the 16-byte loads"
        t = fp.tally(FIT)
        assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
    finally:
        ctx.close()


SIZES = [((5, 3), (5, 3)), ((33, 17), (33, 17)), ((33, 17), (64, 48)), ((64, 48), (33, 17)), ((17, 9), (17, 31)), ((1, 1), (4, 3)), ((9, 1), (3, 5)),
         ((36, 11), (36, 11)), ((36, 11), (64, 13))]


def test_metric_depth_codes_footprint(own_tally):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        vector = 0
        for k, (rng, lays) in enumerate(fp.layout_sweep(8, 1411)):
            (w, h), (ow, oh) = SIZES[k % len(SIZES)]
            if lays.vec:
                (w, h), (ow, oh) = SIZES[7 + k % 2]
            N = 1 + k % 3
            body, (want_codes, want_depth), with_depth, tag = _codes_case(L, ctx, rng, N, h, w, ow, oh, lays, k)
            out, vec = _accept_codes(CODES, body, with_depth, k, tag)
            fp.accepted(CODES, vector=vec)
            vector += int(vec)
            assert np.array_equal(out["codes"].reshape(N, oh, ow, 3), want_codes), tag
            if with_depth:
                got = np.ascontiguousarray(out["depth"]).view(F).reshape(N, oh, ow)
                assert mr.same_bits(got, want_depth).size == 0, tag
            if k % 4 == 0:
                fp.refused(CODES, lambda run: body(run, short=True), INVALID, seed=k)
        fp.finish_entry(CODES, need_odd=True, need_padded=True, need_vector=True)
        assert vector >= 2, "no layout reached the 12-byte stores"
        t = fp.tally(CODES)
        assert t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def slab():
    """One sparse slab for the far cases.  The one permitted skip: less than twice the slab free on the device."""
    import torch
    reason = fp.Slab.skip_reason()
    if reason:
        pytest.skip(reason)
    s = fp.Slab()
    yield s
    del s.buf
    torch.cuda.empty_cache()


FAR_STRIDE = 1 << 32                                   # two frames: the second more than 4 GiB behind the first


def test_fit_with_frames_more_than_4_gib_apart(slab):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        for k, fixed in enumerate(((0, 4, 0), (4, 4, 4))):             # the element path, the 16-byte loads
            rng = np.random.default_rng(400 + k)
            N, H, W = 2, 9, (37, 36)[k]
            body, want, tag = _fit_case(L, ctx, rng, N, H, W, fp.Layouts(rng, fixed, vec=bool(k)), 3 * k)

            def far_body(run):
                body(run)
                assert run.vector == bool(k), tag
                far = [a for a in run.arenas.values() if a.n_frames > 1]
                assert len(far) == 3 and all(a.stride > 1 << 32 for a in far)
            with fp.far(fp.Far(slab, "stride", stride_unit=FAR_STRIDE)):
                out = fp.twice(FIT, far_body, seed=k, what=tag + " [far stride]")
            got = np.ascontiguousarray(out["out"]).view(F).reshape(8)
            assert mr.same_bits(got, want).size == 0, f"{tag}: {got} vs {want}"
    finally:
        ctx.close()


def test_codes_with_frames_more_than_4_gib_apart(slab):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        for k, (fixed, size) in enumerate((((1, 3, 1), ((33, 9), (33, 9))), ((4, 4, 4), ((36, 11), (64, 13))))):
            rng = np.random.default_rng(410 + k)
            (w, h), (ow, oh) = size
            body, (want_codes, want_depth), with_depth, tag = _codes_case(L, ctx, rng, 2, h, w, ow, oh, fp.Layouts(rng, fixed, vec=bool(k)), 3 * k)
            assert with_depth

            def far_body(run):
                body(run)
                far = [a for a in run.arenas.values() if a.n_frames > 1]
                assert len(far) == 3 and all(a.stride > 1 << 32 for a in far)
            with fp.far(fp.Far(slab, "stride", stride_unit=FAR_STRIDE)):
                out = fp.twice(CODES, far_body, seed=k, what=tag + " [far stride]")
            assert np.array_equal(out["codes"].reshape(2, oh, ow, 3), want_codes), tag
            assert mr.same_bits(np.ascontiguousarray(out["depth"]).view(F).reshape(2, oh, ow), want_depth).size == 0, tag
    finally:
        ctx.close()
