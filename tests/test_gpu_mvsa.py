"""The three entry points of include/mdvt_mvsa.h through the raw C ABI, bit for bit against tests/mvsa_ref.py (NumPy on the test machine),
in the arenas of tests/footprint.py -- every output in poison, each case run on a poison and on its complement, so nothing outside an
output's payload changes, every payload byte is written and no byte behind an input row's end matters -- with aligned layouts (the
vector stores), padded pitches, gapped strides and bases one element off (the element paths).  mdvt_bilinear_model_frames at
identities, exact and inexact scales on both sides of torch's own kernel switch, also within the derived bound of torch's CPU
F.interpolate; mdvt_nearest_depth_codes with every special value and factor; mdvt_ratio_median with counts around the histogram's
digits, ratios that differ in one byte only, and launch sets; every refusal, which leaves its text and writes nothing."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import geometry_cases as gc
import metric_align_ref as mr
import mvsa_ref as vr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
F = np.float32
BILINEAR, NEAREST, MEDIAN = "mdvt_bilinear_model_frames", "mdvt_nearest_depth_codes", "mdvt_ratio_median"


def _vp(a):
    return C.c_void_p(a.ptr)


def _moved(name, by):
    """The argument `name`, a pointer, `by` bytes further on."""
    return lambda a: C.c_void_p(a[name].value + by)


def _apply(a, wrong):
    a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})          # (a callable makes its wrong value from the right ones)


@pytest.fixture(scope="module")
def lib():
    """The binding.  The arenas are torch tensors: torch opens the device before the library's context does, as in the rest of the
    suite."""
    import torch
    torch.cuda.init()
    from metric_depth_video_toolbox_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0, 16, 16)
    yield c
    c.close()
    for e in (BILINEAR, NEAREST, MEDIAN):
        fp.TALLY.pop(e, None)                          # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


# layouts (input, output): u8 inputs in bytes; float planes in bytes, kept multiples of 4 (a float32 lies at its alignment)
ALIGNED = (fp.Layout(0, 0, 0), fp.Layout(0, 0, 0))                      # tight: every vector path where the width allows
PADDED16 = (fp.Layout(4, 8, 12), fp.Layout(0, 16, 32))                  # padded pitches, gapped strides, still multiples of 16
ODD = (fp.Layout(1, 3, 5), fp.Layout(4, 12, 20))                        # one element off: the element paths
LAYOUTS = (ALIGNED, PADDED16, ODD)


# ---- mdvt_bilinear_model_frames ---------------------------------------------------------------------------------------------------
def _bilinear_body(lib, ctx, frames, out_size, bgr, lays, plane_gap):
    """frames [N, H, W, 3] as stored.  The output arena holds [N, 3, h, w]: plane_gap puts the layout's gap between planes (frames
    then follow at 3 plane strides), else between frames (planes tight)."""
    L = lib.load()
    N, H, W = frames.shape[:3]
    w, h = out_size
    lin, lout = lays

    def body(run, **wrong):
        ain = run.inp("frames", frames, lin)
        if plane_gap:
            aout = run.out("out", h, 4 * w, 3 * N, lout)
            pitch, plane, stride = aout.pitch, aout.stride, 3 * aout.stride
        else:
            aout = run.out("out", 3 * h, 4 * w, N, lout)
            pitch, plane, stride = aout.pitch, h * aout.pitch, aout.stride
        a = dict(ctx=ctx.handle, in_w=W, in_h=H, n=N, frames=_vp(ain), frames_pitch=ain.pitch, frames_stride=ain.stride, order=int(bgr),
                 out_w=w, out_h=h, out=_vp(aout), out_pitch=pitch, out_plane_stride=plane, out_stride=stride)
        _apply(a, wrong)
        rc = L.mdvt_bilinear_model_frames(a["ctx"], a["in_w"], a["in_h"], a["n"], a["frames"], a["frames_pitch"], a["frames_stride"], a["order"],
                                          a["out_w"], a["out_h"], a["out"], a["out_pitch"], a["out_plane_stride"], a["out_stride"], None)
        if not wrong:
            ctx.check(rc)
        run.vector = fp.all_aligned([aout], 16) and w >= 4
        return rc
    return body


# out_w + out_h <= 128 is torch's kernel for small outputs, above it the two-pass form: both sides of the switch, and 128 and 129
BILINEAR_SIZES = {
    "identity": [((13, 5), (13, 5)), ((16, 9), (16, 9)), ((125, 4), (125, 4))],
    "inexact_up": [((17, 9), (28, 14)), ((17, 9), (121, 8))],
    "inexact_down": [((17, 9), (13, 5)), ((150, 7), (128, 3))],
    "exact": [((15, 9), (8, 4)), ((18, 9), (16, 8)), ((240, 9), (128, 4))],
    "widths_around_the_store": [((9, 5), (3, 2)), ((9, 5), (4, 3)), ((9, 5), (5, 3)), ((20, 9), (17, 6)), ((30, 7), (124, 4)), ((30, 7), (125, 4))],
}


@pytest.mark.parametrize("kind", sorted(BILINEAR_SIZES))
def test_bilinear_frames_equal_the_restatement_and_keep_their_footprint(lib, ctx, kind):
    import torch
    import torch.nn.functional as TF
    vector = cases = 0
    for s, ((W, H), (w, h)) in enumerate(BILINEAR_SIZES[kind]):
        rng = np.random.default_rng(2400 + 10 * sorted(BILINEAR_SIZES).index(kind) + s)
        rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        rgb[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 1], [1, 254, 255]]
        want = vr.bilinear_model_frames(rgb, (w, h))                                    # computed once, shared
        t = torch.from_numpy(rgb).permute(0, 3, 1, 2).float() / 255.0
        torchs = TF.interpolate(t, size=(h, w), mode="bilinear", align_corners=False).numpy()
        B = vr.bilinear_bound(W, H)
        for k, (lays, N, bgr) in enumerate((lays, N, bgr) for lays in LAYOUTS for N in (1, 3) for bgr in (0, 1)):
            stored = np.ascontiguousarray(rgb[:N, ..., ::-1] if bgr else rgb[:N])
            body = _bilinear_body(lib, ctx, stored, (w, h), bgr, lays, plane_gap=k % 2 == 0)
            box = {}

            def accepted(run):
                body(run)
                box["vector"] = run.vector
            tag = f"{kind} {N}x{W}x{H}->{w}x{h} bgr={bgr} {lays}"
            out = fp.twice(BILINEAR, accepted, seed=k, what=tag)["out"]
            fp.accepted(BILINEAR, vector=box["vector"])
            assert box["vector"] or not (lays is ALIGNED and w % 4 == 0), tag           # tight rows of whole groups take the 16-byte stores
            assert not (box["vector"] and lays is ODD), tag
            vector, cases = vector + int(box["vector"]), cases + 1
            got = np.ascontiguousarray(out).view(F).reshape(N, 3, h, w)
            assert mr.same_bits(got, want[:N]).size == 0, tag
            worst = float(np.abs(got.astype(np.float64) - torchs[:N]).max())
            assert worst <= B, f"{tag}: {worst:.3e} from torch's CPU F.interpolate, B = {B:.3e}"
        if (W, H) == (w, h):
            assert mr.same_bits(want, rgb.transpose(0, 3, 1, 2).astype(F) / F(255)).size == 0
    assert vector >= 4 and cases - vector >= 4, "both the vector stores and the element path ran"
    fp.finish_entry(BILINEAR, need_odd=True, need_padded=True, need_vector=True)


# ---- mdvt_nearest_depth_codes -----------------------------------------------------------------------------------------------------
SPECIALS = np.array([np.nan, np.inf, 3.5, -np.inf, 2.25, -1.5, -0.0, 0.0, 1e-40, 250.0, 19.999999, 7.0, 20.0, 100.0, 6.9999995], F)


def _depths(rng, N, h, w, max_depth):
    """Depths in [0, 1.3 max_depth) with, every fifth value, one of SPECIALS: NaN and both infinities, negatives, -0, a denormal,
    values above and at max_depth."""
    x = (rng.random((N, h, w), dtype=F) * F(1.3 * max_depth)).astype(F)
    flat = x.reshape(-1)
    flat[::5] = np.resize(SPECIALS, flat[::5].size)
    return x


def _nearest_body(lib, ctx, x, mid, out_size, max_depth, bgr, scales, scale_stride, plane, lays):
    """x [N, H, W] float32; scales None or float32 [N] (scale_stride 4) or [1] (scale_stride 0)."""
    L = lib.load()
    N, H, W = x.shape
    w, h = out_size
    _, lf = lays
    lcodes = fp.Layout(lays[0].base, lays[0].pad, lays[0].gap)

    def body(run, **wrong):
        ain = run.inp("depth", x, lf)
        asc = run.inp("scale", np.asarray(scales, F).reshape(1, 1, -1), fp.Layout(lf.base)) if scales is not None else None
        acodes = run.out("codes", h, 3 * w, N, lcodes)
        aplane = run.out("plane", h, 4 * w, N, lf) if plane else None
        a = dict(ctx=ctx.handle, in_w=W, in_h=H, n=N, depth=_vp(ain), depth_pitch=ain.pitch, depth_stride=ain.stride, mid_w=mid[0], mid_h=mid[1],
                 scale=_vp(asc) if asc else C.c_void_p(None), scale_stride=scale_stride, max_depth=float(max_depth), out_w=w, out_h=h,
                 codes=_vp(acodes), codes_pitch=acodes.pitch, codes_stride=acodes.stride, order=int(bgr),
                 plane=_vp(aplane) if aplane else C.c_void_p(None), plane_pitch=aplane.pitch if aplane else 0, plane_stride=aplane.stride if aplane else 0)
        _apply(a, wrong)
        rc = L.mdvt_nearest_depth_codes(a["ctx"], a["in_w"], a["in_h"], a["n"], a["depth"], a["depth_pitch"], a["depth_stride"], a["mid_w"],
                                        a["mid_h"], a["scale"], a["scale_stride"], a["max_depth"], a["out_w"], a["out_h"], a["codes"],
                                        a["codes_pitch"], a["codes_stride"], a["order"], a["plane"], a["plane_pitch"], a["plane_stride"], None)
        if not wrong:
            ctx.check(rc)
        run.vector = fp.all_aligned([acodes], 4) and (aplane is None or fp.all_aligned([aplane], 16)) and w >= 4
        return rc
    return body


# (in_w, in_h) -> (mid_w, mid_h) -> (out_w, out_h): up twice, the same size throughout, down twice; then the widths around the store
NEAREST_TRIPLES = [((5, 3), (7, 4), (16, 9)), ((16, 9), (16, 9), (16, 9)), ((17, 9), (13, 5), (6, 4)),
                   ((5, 3), (7, 4), (3, 2)), ((5, 3), (2, 2), (4, 3)), ((9, 4), (7, 3), (5, 2)), ((6, 5), (9, 4), (17, 3))]
FACTORS = (None, 1.0, 0.5, 0.0, np.nan)


@pytest.mark.parametrize("triple", NEAREST_TRIPLES, ids=lambda t: "-".join(f"{w}x{h}" for w, h in t))
def test_nearest_codes_equal_the_restatement_and_keep_their_footprint(lib, ctx, triple):
    (W, H), mid, (w, h) = triple
    rng = np.random.default_rng(2500 + 7 * W + w)
    vector = cases = 0
    for k, (lays, N, bgr) in enumerate((lays, N, bgr) for lays in LAYOUTS for N in (1, 3) for bgr in (0, 1)):
        max_depth = (7, 20, 100)[k % 3]
        x = _depths(rng, N, H, W, max_depth)
        factor = FACTORS[k % len(FACTORS)]
        per_frame = factor is not None and k % 2 == 1 and N > 1
        scales = None if factor is None else np.array([factor, 1.25, 0.75][:N] if per_frame else [factor], F)
        plane = k % 4 != 3
        body = _nearest_body(lib, ctx, x, mid, (w, h), max_depth, bgr, scales, 4 if per_frame else 0, plane, lays)
        box = {}

        def accepted(run):
            body(run)
            box["vector"] = run.vector
        tag = f"{N}x{W}x{H}->{mid}->{w}x{h} bgr={bgr} factor={factor} per_frame={per_frame} plane={plane} max_depth={max_depth} {lays}"
        out = fp.twice(NEAREST, accepted, seed=k, what=tag)
        fp.accepted(NEAREST, vector=box["vector"])
        vector, cases = vector + int(box["vector"]), cases + 1
        full = None if scales is None else np.resize(scales, N)
        want_codes, want_plane = vr.nearest_depth_codes(x, mid, (w, h), max_depth, full, bgr)
        assert np.array_equal(out["codes"].reshape(N, h, w, 3), want_codes), tag
        if plane:
            assert mr.same_bits(np.ascontiguousarray(out["plane"]).view(F).reshape(N, h, w), want_plane).size == 0, tag
    assert (vector >= 2 or w % 4) and cases - vector >= 4, "both the vector stores and the element path ran"
    fp.finish_entry(NEAREST, need_odd=True, need_padded=True, need_vector=w % 4 == 0)


def test_nearest_codes_without_a_factor_are_two_torch_resizes_and_the_sink(lib, ctx):
    """The composition itself, against torch's CPU kernels rather than the restatement: 1024x576 -> 512x288 -> 1920x1080 on one frame."""
    import torch
    import torch.nn.functional as TF
    rng = np.random.default_rng(2550)
    x = (rng.random((1, 576, 1024), dtype=F) * F(120)).astype(F)
    t = torch.from_numpy(x)[None]
    twice = TF.interpolate(TF.interpolate(t, size=(288, 512), mode="nearest"), size=(1080, 1920), mode="nearest")[0].numpy()
    want_plane, want_codes = mr.code(twice[0], 100)
    body = _nearest_body(lib, ctx, x, (512, 288), (1920, 1080), 100, 0, None, 0, True, ALIGNED)
    out = fp.twice(NEAREST, lambda run: body(run), seed=7, what="1080p")
    assert np.array_equal(out["codes"].reshape(1080, 1920, 3), want_codes)
    assert mr.same_bits(np.ascontiguousarray(out["plane"]).view(F).reshape(1080, 1920), want_plane).size == 0


# ---- mdvt_ratio_median ------------------------------------------------------------------------------------------------------------
def _median_body(lib, ctx, cv, ref, mask, lays, counts=True):
    """cv [N, h, w], ref [N, h', w'] float32, mask uint8 [N, hm, wm] or None."""
    L = lib.load()
    N = cv.shape[0]
    lm, lf = lays

    def body(run, **wrong):
        acv, aref = run.inp("cv", cv, lf), run.inp("ref", ref, lf)
        am = run.inp("mask", mask, lm) if mask is not None else None
        amed = run.out("median", 1, 4 * N, 1, fp.Layout(lf.base))
        acnt = run.out("counts", 1, 4 * N, 1, fp.Layout(lf.base)) if counts else None
        a = dict(ctx=ctx.handle, n=N, cv_w=cv.shape[2], cv_h=cv.shape[1], cv=_vp(acv), cv_pitch=acv.pitch, cv_stride=acv.stride,
                 ref_w=ref.shape[2], ref_h=ref.shape[1], ref=_vp(aref), ref_pitch=aref.pitch, ref_stride=aref.stride,
                 mask_w=mask.shape[2] if am else 0, mask_h=mask.shape[1] if am else 0, mask=_vp(am) if am else C.c_void_p(None),
                 mask_pitch=am.pitch if am else 0, mask_stride=am.stride if am else 0, median=_vp(amed),
                 counts=_vp(acnt) if acnt else C.c_void_p(None))
        _apply(a, wrong)
        rc = L.mdvt_ratio_median(a["ctx"], a["n"], a["cv_w"], a["cv_h"], a["cv"], a["cv_pitch"], a["cv_stride"], a["ref_w"], a["ref_h"],
                                 a["ref"], a["ref_pitch"], a["ref_stride"], a["mask_w"], a["mask_h"], a["mask"], a["mask_pitch"],
                                 a["mask_stride"], a["median"], a["counts"], None)
        if not wrong:
            ctx.check(rc)
        return rc
    return body


def _median_check(lib, ctx, cv, ref, mask, lays, seed, tag, counts=True):
    want_med, want_cnt = vr.ratio_median(cv, ref, mask)
    out = fp.twice(MEDIAN, lambda run: _median_body(lib, ctx, cv, ref, mask, lays, counts)(run), seed=seed, what=tag)
    fp.accepted(MEDIAN)
    assert mr.same_bits(np.ascontiguousarray(out["median"]).view(F).reshape(-1), want_med).size == 0, (tag, out["median"].view(F), want_med)
    if counts:
        assert np.array_equal(np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(-1), want_cnt), tag
    return want_med, want_cnt


COUNTS = (0, 1, 2, 255, 256, 257, 9215, 9216, 9217)


def _counted_frame(rng, count, h=96, w=97):
    """A frame of 9312 pixels with exactly `count` valid ratios scattered over it; the others fail each in its own way."""
    cv = rng.uniform(0.1, 50.0, (h, w)).astype(F)
    ref = rng.uniform(0.1, 50.0, (h, w)).astype(F)
    bad = rng.permutation(h * w)[count:]
    half = bad.size // 2
    cv.reshape(-1)[bad[:half]] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, -np.inf, -0.0], F), half)
    ref.reshape(-1)[bad[half:]] = np.resize(np.array([0.0, -2.0, np.nan, np.inf, -np.inf, -0.0], F), bad.size - half)
    return cv, ref


def test_median_counts_around_a_digit_and_a_frame(lib, ctx):
    rng = np.random.default_rng(2600)
    frames = [_counted_frame(rng, c) for c in COUNTS]
    for k, (cv, ref) in enumerate(frames):                           # one frame per call
        _, cnt = _median_check(lib, ctx, cv[None], ref[None], None, LAYOUTS[k % 3], k, f"count {COUNTS[k]}")
        assert cnt[0] == COUNTS[k]
    cv, ref = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    med, cnt = _median_check(lib, ctx, cv, ref, None, PADDED16, 50, "nine frames with different counts in one call")
    assert cnt.tolist() == list(COUNTS) and med[0] == F(1)
    _median_check(lib, ctx, cv[[8, 0, 4]], ref[[8, 0, 4]], None, ODD, 51, "three frames with different counts in one call", counts=False)
    fp.finish_entry(MEDIAN, need_odd=False, need_padded=True)


def test_median_where_every_radix_pass_decides_once(lib, ctx):
    """ref = 64 makes ref + 1e-6 = 64 and cv / 64 exact, so the ratios' bits are the test's to choose."""
    rng = np.random.default_rng(2601)

    def frame(bits):
        r = np.array(bits, np.uint32).view(F)
        cv = np.full((16, 16), -1.0, F)                             # invalid but for the chosen ones
        cv.reshape(-1)[rng.permutation(256)[:r.size]] = r * F(64)
        return cv, np.full((16, 16), 64.0, F)
    low = frame([0x3F800000 | k for k in range(256)])               # differ in the lowest byte only: the last pass decides
    high = frame([(k << 24) | 0x00123456 for k in range(1, 0x7C)])  # differ in the highest byte only: the first pass decides
    second = frame([0x40000012 | (k << 16) for k in range(0x7F)])   # in the second byte only
    third = frame([0x40490034 | (k << 8) for k in range(200)])      # in the third byte only
    equal = frame([0x40490FDB] * 77)
    for k, (cv, ref) in enumerate((low, high, second, third, equal)):
        ratios = vr.valid_ratios(cv, ref).view(np.uint32)
        assert ratios.size == (256, 0x7B, 0x7F, 200, 77)[k]
        med, _ = _median_check(lib, ctx, cv[None], ref[None], None, ALIGNED, 60 + k, f"one-byte case {k}")
        assert med.view(np.uint32)[0] == np.sort(ratios)[(ratios.size - 1) // 2]
    assert vr.ratio_median(low[0][None], low[1][None])[0].view(np.uint32)[0] == 0x3F80007F
    cv, ref = np.stack([f[0] for f in (low, high, second, third, equal)]), np.stack([f[1] for f in (low, high, second, third, equal)])
    _median_check(lib, ctx, cv, ref, None, PADDED16, 66, "the five in one call")
    # +inf is a ratio like any other, above every finite one
    cv, ref = np.full((1, 3, 3), -1.0, F), np.full((1, 3, 3), 1e-3, F)
    cv[0, 0, :3] = [3e38, 2.0, 3e38]
    med, cnt = _median_check(lib, ctx, cv, ref, None, ALIGNED, 67, "two infinities and a finite ratio")
    assert cnt[0] == 3 and np.isposinf(med[0])


def test_median_samples_the_refined_depth_and_the_mask_through_the_nearest_map(lib, ctx):
    rng = np.random.default_rng(2602)
    for k, (cv_s, ref_s, mask_s) in enumerate([((9, 14), (18, 28), (9, 14)), ((9, 14), (5, 9), (4, 7)), ((17, 13), (17, 13), (40, 33)),
                                               ((6, 5), (13, 17), (1, 1))]):
        cv = rng.uniform(-1.0, 50.0, (3,) + cv_s).astype(F)
        ref = rng.uniform(-1.0, 50.0, (3,) + ref_s).astype(F)
        mask = (rng.random((3,) + mask_s) < 0.6).astype(np.uint8) * rng.integers(1, 256, (3,) + mask_s).astype(np.uint8)
        _, cnt = _median_check(lib, ctx, cv, ref, mask, LAYOUTS[k % 3], 70 + k, f"cv {cv_s} ref {ref_s} mask {mask_s}")
        assert mask_s == (1, 1) or (0 < cnt.min() and cnt.max() < cv_s[0] * cv_s[1])
    zero = np.zeros((3, 2, 2), np.uint8)
    med, cnt = _median_check(lib, ctx, cv, ref, zero, ALIGNED, 79, "a mask that is false everywhere")
    assert cnt.tolist() == [0, 0, 0] and med.tolist() == [1.0, 1.0, 1.0]


def test_median_runs_in_two_launch_sets_under_a_small_workspace(lib):
    """workspace_mib = 1 affords 1008 frames of 1040 B: 1100 frames are two launch sets, on a block of 1008 frames' scratch."""
    import torch
    rng = np.random.default_rng(2603)
    N = 1100
    cv = rng.uniform(-5.0, 50.0, (N, 4, 5)).astype(F)
    ref = rng.uniform(0.1, 50.0, (N, 3, 3)).astype(F)
    want_med, want_cnt = vr.ratio_median(cv, ref)
    assert len(set(want_cnt.tolist())) > 3
    ctx = gc.make_context(lib, 16, 16, workspace_mib=1)
    try:
        before = ctx.workspace_bytes()
        d_cv, d_ref = torch.from_numpy(cv).cuda(), torch.from_numpy(ref).cuda()
        med, cnt = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        ctx.check(lib.load().mdvt_ratio_median(ctx.handle, N, 5, 4, d_cv.data_ptr(), 20, 80, 3, 3, d_ref.data_ptr(), 12, 36, 0, 0, None, 0, 0,
                                               med.data_ptr(), cnt.data_ptr(), None))
        torch.cuda.synchronize()
        per_set = (1 << 20) // 1040
        assert per_set < N <= 2 * per_set and 0 < ctx.workspace_bytes() - before <= 1 << 20, "a block within the budget: exactly two launch sets"
        assert mr.same_bits(med.cpu().numpy(), want_med).size == 0 and np.array_equal(cnt.cpu().numpy().view(np.uint32), want_cnt)
    finally:
        ctx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(lib, ctx, entry, body, cases):
    L = lib.load()
    for k, (what, wrong, status, text) in enumerate(cases):
        fp.refused(entry, lambda run: body(run, **wrong), status, seed=k)
        got = (L.mdvt_last_error(ctx.handle) or b"").decode()
        assert text in got, f"{entry}, {what}: mdvt_last_error says {got!r}"
    assert fp.tally(entry)["refused"] >= len(cases)


def test_bilinear_refusals_leave_their_text_and_write_nothing(lib, ctx):
    rng = np.random.default_rng(2700)
    N, (W, H), (w, h) = 2, (9, 5), (12, 7)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    none = C.c_void_p(None)
    body = _bilinear_body(lib, ctx, frames, (w, h), 0, ALIGNED, plane_gap=False)
    text = "must be multiples of 4"
    cases = [("NULL frames", dict(frames=none), INVALID, "NULL buffer"), ("NULL out", dict(out=none), INVALID, "NULL buffer"),
             ("in_w 0", dict(in_w=0), INVALID, "bad size"), ("in_h -1", dict(in_h=-1), INVALID, "bad size"),
             ("out_w 0", dict(out_w=0), INVALID, "bad size"), ("out_h 0", dict(out_h=0), INVALID, "bad size"),
             ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"), ("order 2", dict(order=2), INVALID, "order must be"),
             ("order -1", dict(order=-1), INVALID, "order must be"),
             ("a short frames pitch", dict(frames_pitch=3 * W - 1), INVALID, "frames_pitch smaller than one row"),
             ("a short out pitch", dict(out_pitch=4 * w - 4), INVALID, "out_pitch smaller than one row"),
             ("a short plane stride", dict(out_plane_stride=4 * w * h - 4), INVALID, "out_plane_stride smaller than one plane"),
             ("a short frames stride", dict(frames_stride=3 * W * H - 1), INVALID, "stride smaller than one frame"),
             ("a short out stride", dict(out_stride=3 * 4 * w * h - 4), INVALID, "stride smaller than one frame"),
             ("an out pitch of 4 w + 1", dict(out_pitch=4 * w + 1, out_plane_stride=(4 * w + 4) * h, out_stride=3 * (4 * w + 4) * h), INVALID, text),
             ("a plane stride off by 2", dict(out_plane_stride=4 * w * h + 2, out_stride=3 * (4 * w * h + 4)), INVALID, text),
             ("an out stride off by 1", dict(out_stride=3 * 4 * w * h + 1), INVALID, text),
             ("d_out off by 1", dict(out=_moved("out", 1)), INVALID, text), ("d_out off by 2", dict(out=_moved("out", 2)), INVALID, text),
             ("2^31 output pixels", dict(out_w=1 << 16, out_h=1 << 15, out_pitch=4 << 16, out_plane_stride=4 << 31, out_stride=3 * 4 << 31),
              UNSUPPORTED, "frame too large"),
             ("2^31 input pixels", dict(in_w=1 << 16, in_h=1 << 15, frames_pitch=3 << 16, frames_stride=3 << 31), UNSUPPORTED, "frame too large")]
    _refused(lib, ctx, BILINEAR, body, cases)
    fp.twice(BILINEAR, lambda run: body(run), seed=99)              # the context still works after them


def test_nearest_refusals_leave_their_text_and_write_nothing(lib, ctx):
    rng = np.random.default_rng(2701)
    N, (W, H), mid, (w, h) = 2, (9, 5), (7, 4), (12, 7)
    x = _depths(rng, N, H, W, 20)
    none = C.c_void_p(None)
    body = _nearest_body(lib, ctx, x, mid, (w, h), 20, 0, np.array([0.5, 2.0], F), 4, True, ALIGNED)
    text = "must be multiples of 4"
    cases = [("NULL depth", dict(depth=none), INVALID, "NULL buffer"), ("NULL codes", dict(codes=none), INVALID, "NULL buffer"),
             ("in_w 0", dict(in_w=0), INVALID, "bad size"), ("in_h 0", dict(in_h=0), INVALID, "bad size"),
             ("mid_w 0", dict(mid_w=0), INVALID, "bad size"), ("mid_h -1", dict(mid_h=-1), INVALID, "bad size"),
             ("out_w 0", dict(out_w=0), INVALID, "bad size"), ("out_h 0", dict(out_h=0), INVALID, "bad size"),
             ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"), ("order 2", dict(order=2), INVALID, "order must be"),
             ("max_depth 0", dict(max_depth=0.0), INVALID, "max_depth must be > 0"),
             ("max_depth NaN", dict(max_depth=float("nan")), INVALID, "max_depth must be > 0"),
             ("max_depth -1", dict(max_depth=-1.0), INVALID, "max_depth must be > 0"),
             ("a short depth pitch", dict(depth_pitch=4 * W - 4), INVALID, "depth_pitch smaller than one row"),
             ("a short codes pitch", dict(codes_pitch=3 * w - 1), INVALID, "codes_pitch smaller than one row"),
             ("a short plane pitch", dict(plane_pitch=4 * w - 4), INVALID, "plane_pitch smaller than one row"),
             ("a short depth stride", dict(depth_stride=4 * W * H - 4), INVALID, "stride smaller than one frame"),
             ("a short codes stride", dict(codes_stride=3 * w * h - 1), INVALID, "stride smaller than one frame"),
             ("a short plane stride", dict(plane_stride=4 * w * h - 4), INVALID, "stride smaller than one frame"),
             ("a depth pitch off by 2", dict(depth_pitch=4 * W + 2, depth_stride=(4 * W + 4) * H), INVALID, text),
             ("d_depth off by 1", dict(depth=_moved("depth", 1)), INVALID, text),
             ("d_plane off by 2", dict(plane=_moved("plane", 2)), INVALID, text),
             ("a plane stride off by 2", dict(plane_stride=4 * w * h + 2), INVALID, text),
             ("d_scale off by 2", dict(scale=_moved("scale", 2)), INVALID, "d_scale and scale_stride"),
             ("a scale stride of 3", dict(scale_stride=3), INVALID, "d_scale and scale_stride"),
             ("2^31 output pixels", dict(out_w=1 << 16, out_h=1 << 15, codes_pitch=3 << 16, codes_stride=3 << 31, plane_pitch=4 << 16,
                                         plane_stride=4 << 31), UNSUPPORTED, "output frame too large")]
    _refused(lib, ctx, NEAREST, body, cases)
    out = fp.twice(NEAREST, lambda run: body(run), seed=99)         # the context still works after them
    assert np.array_equal(out["codes"].reshape(N, h, w, 3), vr.nearest_depth_codes(x, mid, (w, h), 20, np.array([0.5, 2.0], F))[0])


def test_median_refusals_leave_their_text_and_write_nothing(lib, ctx):
    rng = np.random.default_rng(2702)
    N = 2
    cv, ref = rng.uniform(0.1, 9.0, (N, 5, 9)).astype(F), rng.uniform(0.1, 9.0, (N, 4, 6)).astype(F)
    mask = rng.integers(0, 2, (N, 3, 7), dtype=np.uint8)
    none = C.c_void_p(None)
    body = _median_body(lib, ctx, cv, ref, mask, ALIGNED)
    text = "must be multiples of 4"
    cases = [("NULL cv", dict(cv=none), INVALID, "NULL buffer"), ("NULL ref", dict(ref=none), INVALID, "NULL buffer"),
             ("NULL median", dict(median=none), INVALID, "NULL buffer"), ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"),
             ("cv_w 0", dict(cv_w=0), INVALID, "bad size"), ("cv_h -1", dict(cv_h=-1), INVALID, "bad size"),
             ("ref_w 0", dict(ref_w=0), INVALID, "bad size"), ("ref_h 0", dict(ref_h=0), INVALID, "bad size"),
             ("mask_w 0", dict(mask_w=0), INVALID, "bad mask size"), ("mask_h 0", dict(mask_h=0), INVALID, "bad mask size"),
             ("a short cv pitch", dict(cv_pitch=4 * 9 - 4), INVALID, "cv_pitch smaller than one row"),
             ("a short ref pitch", dict(ref_pitch=4 * 6 - 4), INVALID, "ref_pitch smaller than one row"),
             ("a short mask pitch", dict(mask_pitch=6), INVALID, "mask_pitch smaller than one row"),
             ("a short cv stride", dict(cv_stride=4 * 9 * 5 - 4), INVALID, "stride smaller than one frame"),
             ("a short ref stride", dict(ref_stride=4 * 6 * 4 - 4), INVALID, "stride smaller than one frame"),
             ("a short mask stride", dict(mask_stride=7 * 3 - 1), INVALID, "stride smaller than one frame"),
             ("a cv pitch off by 2", dict(cv_pitch=4 * 9 + 2, cv_stride=(4 * 9 + 4) * 5), INVALID, text),
             ("a ref stride off by 1", dict(ref_stride=4 * 6 * 4 + 1), INVALID, text),
             ("d_cv off by 1", dict(cv=_moved("cv", 1)), INVALID, text), ("d_ref off by 2", dict(ref=_moved("ref", 2)), INVALID, text),
             ("d_median off by 2", dict(median=_moved("median", 2)), INVALID, "4-byte aligned"),
             ("d_counts off by 1", dict(counts=_moved("counts", 1)), INVALID, "4-byte aligned"),
             ("2^31 pixels", dict(cv_w=1 << 16, cv_h=1 << 15, cv_pitch=4 << 16, cv_stride=4 << 31), UNSUPPORTED, "cost volume too large")]
    _refused(lib, ctx, MEDIAN, body, cases)
    out = fp.twice(MEDIAN, lambda run: body(run), seed=99)          # the context still works; both outputs are written
    want_med, want_cnt = vr.ratio_median(cv, ref, mask)
    assert mr.same_bits(np.ascontiguousarray(out["median"]).view(F).reshape(-1), want_med).size == 0
    assert np.array_equal(np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(-1), want_cnt)
