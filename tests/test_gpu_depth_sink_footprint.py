"""mdvt_depth_video_codes (include/mdvt_depth_sink.h) held to its footprint with the arenas of tests/footprint.py, through the raw C
ABI: the call writes the first 3 * out_w bytes of each code row and the first 4 * out_w bytes of each plane row, nothing else; every
one of those bytes is written; the result does not depend on the bytes behind an input row's end (each case runs on a poison and on
its complement); a refused call leaves everything as it was; and one case has its frames more than 4 GiB apart, for the input, the
codes and the planes.  Expected values: tests/depth_sink_ref.py, bit for bit.  (The entry point is declared outside include/mdvt.h,
so its case family lives here; its tally row is printed here and taken out of the shared table again.)"""
import ctypes as C

import numpy as np
import pytest

import depth_sink_ref as dr
import footprint as fp
import metric_align_ref as mr

pytestmark = pytest.mark.gpu

SINK = "mdvt_depth_video_codes"
INVALID, UNSUPPORTED = -1, -3
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
        fp.TALLY.pop(SINK, None)                       # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def _case(L, ctx, rng, N, h, w, ow, oh, lays, k):
    """-> (body(run, **wrong), (codes, planes), with_plane, tag).  wrong: one argument replaced by a value the header refuses."""
    order, with_plane, with_scale, ntm = (k // 2) % 2, k % 3 != 2, k % 2 == 0, (k // 3) % 2
    scale, max_depth = (0.75, 20) if k % 4 < 2 else (1.2345678, 100)
    x = (rng.random((N, h, w), dtype=F) * F(1.3 * max_depth)).astype(F)
    x.reshape(-1)[::7] = np.resize(np.array([np.nan, -2.0, -0.0, 250.0, 1e-40], F), x.reshape(-1)[::7].size)
    want = dr.sink(x, max_depth, (ow, oh), scale if with_scale else None, bool(ntm), bool(order))
    lx, lc, lp, ls = lays.w32(), lays.u8(), lays.w32(), lays.w32()

    def body(run, **wrong):
        ax = run.inp("depth", x, lx)
        asc = run.inp("scale", np.array([[[scale]]], F), fp.Layout(ls.base))
        ac = run.out("codes", oh, 3 * ow, N, lc)
        ap = run.out("plane", oh, 4 * ow, N, lp)
        a = dict(ctx=ctx.handle, in_w=w, in_h=h, n=N, depth=_vp(ax), depth_pitch=ax.pitch, depth_stride=ax.stride,
                 scale=_vp(asc) if with_scale else None, nan_to_max=ntm, max_depth=float(max_depth), out_w=ow, out_h=oh,
                 codes=_vp(ac), codes_pitch=ac.pitch, codes_stride=ac.stride, order=order,
                 plane=_vp(ap) if with_plane else None, plane_pitch=ap.pitch, plane_stride=ap.stride)
        a.update(wrong)
        rc = L.mdvt_depth_video_codes(a["ctx"], a["in_w"], a["in_h"], a["n"], a["depth"], a["depth_pitch"], a["depth_stride"], a["scale"],
                                      a["nan_to_max"], a["max_depth"], a["out_w"], a["out_h"], a["codes"], a["codes_pitch"], a["codes_stride"],
                                      a["order"], a["plane"], a["plane_pitch"], a["plane_stride"], None)
        if not wrong:
            ctx.check(rc)
        run.vector = fp.all_aligned([ac], 4) and ow >= 4                       # the 12-byte stores of four codes
        run.vector_loads = (w, h) == (ow, oh) and w >= 4 and fp.all_aligned([ax], 16)
        return rc
    tag = f"sink {N}x{w}x{h}->{ow}x{oh} order={order} scale={with_scale} nan_to_max={ntm} plane={with_plane} {lx} {lc} {lp}"
    return body, want, with_plane, tag


def _accept(body, with_plane, seed, tag):
    box = {}

    def body_accepted(run):
        body(run)
        if not with_plane:                             # d_plane NULL: the arena stays poison, as an input would
            run.arenas["plane"].input = run.arenas["plane"].payload(run.arenas["plane"].poison)
        box["vector"], box["loads"] = run.vector, run.vector_loads
    out = fp.twice(SINK, body_accepted, seed=seed, what=tag)
    return out, box["vector"], box["loads"]


SIZES = [((5, 3), (5, 3)), ((33, 17), (33, 17)), ((33, 17), (64, 48)), ((64, 48), (33, 17)), ((17, 9), (17, 31)), ((1, 1), (4, 3)), ((9, 1), (3, 5)),
         ((36, 11), (36, 11)), ((36, 11), (64, 13))]


def test_depth_video_codes_footprint(own_tally):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        vector = loads = 0
        for k, (rng, lays) in enumerate(fp.layout_sweep(8, 1710)):
            (w, h), (ow, oh) = SIZES[k % len(SIZES)]
            if lays.vec:
                (w, h), (ow, oh) = SIZES[7 + k % 2]
            N = 1 + k % 3
            body, (want_codes, want_plane), with_plane, tag = _case(L, ctx, rng, N, h, w, ow, oh, lays, k)
            out, vec, ld = _accept(body, with_plane, k, tag)
            fp.accepted(SINK, vector=vec)
            vector, loads = vector + int(vec), loads + int(ld)
            assert np.array_equal(out["codes"].reshape(N, oh, ow, 3), want_codes), tag
            if with_plane:
                got = np.ascontiguousarray(out["plane"]).view(F).reshape(N, oh, ow)
                assert mr.same_bits(got, want_plane).size == 0, tag
        fp.finish_entry(SINK, need_odd=True, need_padded=True, need_vector=True)
        assert vector >= 2, "no layout reached the 12-byte stores"
        assert loads >= 1, "no layout reached the 16-byte loads"
        t = fp.tally(SINK)
        assert t["outside_bytes"] >= 2 * 4096 * t["accepted"]
    finally:
        ctx.close()


# every argument the header refuses: MDVT_ERR_INVALID_ARG, and MDVT_ERR_UNSUPPORTED for a frame of 2^31 pixels
def _refusals(N, h, w, ow, oh):
    none = C.c_void_p(None)
    out = [("a NULL depth", dict(depth=none), INVALID), ("NULL codes", dict(codes=none), INVALID),
           ("in_w 0", dict(in_w=0), INVALID), ("in_h 0", dict(in_h=0), INVALID), ("out_w 0", dict(out_w=0), INVALID),
           ("out_h -1", dict(out_h=-1), INVALID), ("no frame", dict(n=0), INVALID),
           ("a short depth pitch", dict(depth_pitch=4 * w - 4), INVALID), ("a short codes pitch", dict(codes_pitch=3 * ow - 1), INVALID),
           ("a short plane pitch", dict(plane_pitch=4 * ow - 4), INVALID),
           ("order 2", dict(order=2), INVALID), ("nan_to_max 2", dict(nan_to_max=2), INVALID), ("nan_to_max -1", dict(nan_to_max=-1), INVALID),
           ("max_depth 0", dict(max_depth=0.0), INVALID), ("max_depth NaN", dict(max_depth=float("nan")), INVALID),
           ("max_depth -1", dict(max_depth=-1.0), INVALID),
           ("2^31 pixels", dict(out_w=1 << 16, out_h=1 << 15, codes_pitch=3 << 16, plane_pitch=4 << 16, codes_stride=3 << 31, plane_stride=4 << 31),
            UNSUPPORTED)]
    if N > 1:
        out += [("a short depth stride", dict(depth_stride=4 * w * h - 4), INVALID), ("a short codes stride", dict(codes_stride=3 * ow * oh - 1), INVALID),
                ("a short plane stride", dict(plane_stride=4 * ow * oh - 4), INVALID)]
    return out


def test_every_refused_argument_is_refused_untouched(own_tally):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        rng = np.random.default_rng(1711)
        N, (w, h), (ow, oh) = 2, (9, 5), (12, 7)
        body, _, with_plane, tag = _case(L, ctx, rng, N, h, w, ow, oh, fp.Layouts(rng, (0, 0, 0)), 0)
        assert with_plane
        cases = _refusals(N, h, w, ow, oh)
        for k, (what, wrong, status) in enumerate(cases):
            fp.refused(SINK, lambda run: body(run, **wrong), status, seed=k)
        assert L.mdvt_depth_video_codes(None, w, h, 1, None, 4 * w, 0, None, 0, 20.0, ow, oh, None, 3 * ow, 0, 0, None, 0, 0, None) == INVALID
        assert fp.tally(SINK)["refused"] == len(cases) >= 20
        fp.twice(SINK, lambda run: body(run), seed=99, what=tag)       # the context still works after them
    finally:
        ctx.close()


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


def test_frames_more_than_4_gib_apart(slab):
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        for k, (fixed, size) in enumerate((((1, 3, 1), ((33, 9), (33, 9))), ((4, 4, 4), ((36, 11), (36, 11))), ((4, 4, 4), ((36, 11), (64, 13))))):
            rng = np.random.default_rng(1720 + k)
            (w, h), (ow, oh) = size
            body, (want_codes, want_plane), with_plane, tag = _case(L, ctx, rng, 2, h, w, ow, oh, fp.Layouts(rng, fixed, vec=bool(k)), 3 * k)
            assert with_plane

            def far_body(run):
                body(run)
                assert run.vector_loads == (k == 1), tag
                far = [a for a in run.arenas.values() if a.n_frames > 1]
                assert len(far) == 3 and all(a.stride > 1 << 32 for a in far)
            with fp.far(fp.Far(slab, "stride", stride_unit=FAR_STRIDE)):
                out = fp.twice(SINK, far_body, seed=k, what=tag + " [far stride]")
            assert np.array_equal(out["codes"].reshape(2, oh, ow, 3), want_codes), tag
            assert mr.same_bits(np.ascontiguousarray(out["plane"]).view(F).reshape(2, oh, ow), want_plane).size == 0, tag
    finally:
        ctx.close()
