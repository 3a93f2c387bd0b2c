"""The three entry points of include/mdvt_video_mask.h through the raw C ABI, bit for bit against tests/video_mask_ref.py (NumPy on the
test machine; tests/test_video_mask_cpu.py holds that restatement to Pillow itself): every output in the arenas of tests/footprint.py --
in poison, each case run on a poison and on its complement, so nothing outside the first out_w elements of a row changes, every one of
those is written and no byte behind an input row's end matters -- with aligned layouts (the vector stores), padded pitches, gapped
strides and bases one byte off (the element paths), one frame and three; both forms of the resampler, each asserted to have been
taken; noise and 0/255 steps, which drive the filter's negative lobes into both clamps; the decrees; every refusal, which leaves its
text and writes nothing."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import footprint as fp
import geometry_cases as gc
import video_mask_ref as vr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
F = np.float32
RESIZE, INPUT, MASK = "mdvt_lanczos_resize_u8", "mdvt_mask_model_input", "mdvt_mask_from_prediction"
AUTO, FUSED, TWO = 0, 1, 2

# layouts: (input, output)
ALIGNED = (fp.Layout(0, 0, 0), fp.Layout(0, 0, 0))
PADDED16 = (fp.Layout(4, 8, 12), fp.Layout(0, 16, 32))
ODD = (fp.Layout(1, 3, 5), fp.Layout(1, 3, 5))
LAYOUTS = (ALIGNED, PADDED16, ODD)


def _vp(a):
    return C.c_void_p(a.ptr)


def _moved(name, by):
    return lambda a: C.c_void_p(a[name].value + by)


def _f32(lay):
    """A uint8 layout as a float32 plane may have it: everything a multiple of 4 (one byte off becomes four off)."""
    return fp.Layout(lay.base * 4 % 16, lay.pad * 4 if lay.pad % 4 else lay.pad, lay.gap * 4 if lay.gap % 4 else lay.gap)


def _steps(rng, shape):
    """0 / 255 in blocks: edges, whose overshoot reaches both clamps."""
    b = max(1, min(shape[1], shape[2]) // 6)
    cells = rng.integers(0, 2, (shape[0], -(-shape[1] // b), -(-shape[2] // b)) + tuple(shape[3:])) * 255
    return np.repeat(np.repeat(cells, b, axis=1), b, axis=2)[:, :shape[1], :shape[2]].astype(np.uint8)


def _images(seed, n, size, ch):
    """n frames at size = (w, h): noise, steps, noise, ..."""
    rng = np.random.default_rng(seed)
    shape = (n, size[1], size[0]) + ((3,) if ch == 3 else ())
    out = rng.integers(0, 256, shape, dtype=np.uint8)
    out[1::2] = _steps(rng, shape)[1::2]
    return out


def expected_form(src, dst, ch):
    """The header's rule for the library's choice: two launches (the fused form was measured slower), 0 for a copy."""
    return 0 if src == dst else TWO


@pytest.fixture(scope="module")
def lib():
    import torch
    torch.cuda.init()
    from metric_depth_video_toolbox_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0, 16, 16)
    yield c
    c.close()
    for e in (RESIZE, INPUT, MASK):
        fp.TALLY.pop(e, None)                          # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


@pytest.fixture(scope="module")
def tool():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("generate_video_mask_tool", os.path.join(repo, "tools", "generate_video_mask.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- mdvt_lanczos_resize_u8 ---------------------------------------------------------------------------------------------------------
def _resize_body(lib, ctx, images, dst, ch, lays, form):
    L = lib.load()
    N, H, W = images.shape[:3]
    w, h = dst
    lin, lout = lays

    def body(run, **wrong):
        ain = run.inp("in", images.reshape(N, H, W * ch), lin)
        aout = run.out("out", h, ch * w, N, lout)
        took = C.c_int(-7)
        a = dict(ctx=ctx.handle, in_w=W, in_h=H, channels=ch, n=N, d_in=_vp(ain), in_pitch=ain.pitch, in_stride=ain.stride, out_w=w, out_h=h,
                 d_out=_vp(aout), out_pitch=aout.pitch, out_stride=aout.stride, form=form)
        a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})
        rc = L.mdvt_lanczos_resize_u8(a["ctx"], a["in_w"], a["in_h"], a["channels"], a["n"], a["d_in"], a["in_pitch"], a["in_stride"], a["out_w"],
                                      a["out_h"], a["d_out"], a["out_pitch"], a["out_stride"], a["form"], C.byref(took), None)
        if not wrong:
            ctx.check(rc)
        run.took = took.value
        return rc
    return body


def _resize_case(lib, ctx, images, dst, ch, want, forms, tag):
    """Every layout and frame count in every form of `forms`; -> the forms taken."""
    taken = set()
    for k, (lays, N, form) in enumerate((lays, N, form) for lays in LAYOUTS for N in (1, 3) for form in forms):
        box = {}

        def accepted(run):
            _resize_body(lib, ctx, images[:N], dst, ch, lays, form)(run)
            box["took"] = run.took
        what = f"{tag} n={N} form={form} {lays}"
        out = fp.twice(RESIZE, accepted, seed=k, what=what)["out"]
        fp.accepted(RESIZE)
        src = (images.shape[2], images.shape[1])
        assert box["took"] == (form if form and src != dst else expected_form(src, dst, ch)), what
        taken.add(box["took"])
        assert np.array_equal(out.reshape(want[:N].shape), want[:N]), what
    return taken


RGB_SOURCES = [(1, 1), (5, 4), (37, 23), (333, 187), (641, 321), (320, 200), (320, 320)]
L_TARGETS = [(1, 1), (5, 4), (37, 23), (320, 200), (641, 361), (1000, 7)]


@pytest.mark.parametrize("src", RGB_SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_frames_to_the_models_square(lib, ctx, src):
    images = _images(3000 + src[0], 3, src, 3)
    want = vr.lanczos_resize(images, (320, 320), 3)                   # computed once, shared
    shrinks = src[0] > 320 and src[1] > 320
    taken = _resize_case(lib, ctx, images, (320, 320), 3, want, (AUTO, FUSED, TWO) if shrinks else (AUTO, TWO), f"RGB {src}->320x320")
    # 641 x 321 fits the fused form, which runs where it is asked for; the library's own choice is two launches; 320 x 200 runs one pass
    assert taken == ({FUSED, TWO} if shrinks else {0} if src == (320, 320) else {TWO})
    if src == (641, 321):
        assert want.min() == 0 and want.max() == 255                 # the steps reached both clamps
    fp.finish_entry(RESIZE, need_odd=True, need_padded=True)


@pytest.mark.parametrize("dst", L_TARGETS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grey_masks_out_of_the_models_square(lib, ctx, dst):
    images = _images(3100 + dst[0], 3, (320, 320), 1)
    want = vr.lanczos_resize(images, dst, 1)
    shrinks = dst[0] < 320 and dst[1] < 320
    taken = _resize_case(lib, ctx, images, dst, 1, want, (AUTO, FUSED, TWO) if shrinks else (AUTO, TWO), f"L 320x320->{dst}")
    assert taken == ({FUSED, TWO} if shrinks else {TWO})
    fp.finish_entry(RESIZE, need_odd=True, need_padded=True)


def test_the_forms_are_taken_where_the_header_says_and_give_the_same_bits(lib, ctx):
    """A strip that does not fit in LDS forces the two-launch form (the fused form is refused there); with one channel the same strip
    fits and takes the fused form when it is asked for, as does a resize with one axis each way."""
    L = lib.load()
    tall = _images(3200, 1, (12, 2800), 3)                           # 2800 rows x 8 columns x 3 bytes > 64 KiB
    want = vr.lanczos_resize(tall, (5, 40), 3)
    box = {}

    def auto(run):
        _resize_body(lib, ctx, tall, (5, 40), 3, ODD, AUTO)(run)
        box["took"] = run.took
    out = fp.twice(RESIZE, auto, seed=1, what="tall auto")["out"]
    assert box["took"] == TWO and expected_form((12, 2800), (5, 40), 3) == TWO and np.array_equal(out.reshape(want.shape), want)
    fp.refused(RESIZE, lambda run: _resize_body(lib, ctx, tall, (5, 40), 3, ODD, AUTO)(run, form=FUSED), UNSUPPORTED, seed=2)
    assert "the fused form needs both passes" in (L.mdvt_last_error(ctx.handle) or b"").decode()
    grey = np.ascontiguousarray(tall[..., 0])                        # one channel: 2800 x 8 fits
    want = vr.lanczos_resize(grey, (5, 40), 1)
    for form in (AUTO, FUSED, TWO):
        def one(run):
            _resize_body(lib, ctx, grey, (5, 40), 1, PADDED16, form)(run)
            box["took"] = run.took
        out = fp.twice(RESIZE, one, seed=3 + form, what=f"tall grey form {form}")["out"]
        assert box["took"] == (form or TWO) and np.array_equal(out.reshape(want.shape), want), form
    mixed = _images(3201, 3, (45, 20), 3)                            # wider -> narrower, lower -> higher
    want = vr.lanczos_resize(mixed, (19, 33), 3)
    for form, took in ((AUTO, TWO), (FUSED, FUSED), (TWO, TWO)):
        def two(run):
            _resize_body(lib, ctx, mixed, (19, 33), 3, ODD, form)(run)
            box["took"] = run.took
        out = fp.twice(RESIZE, two, seed=7 + form, what=f"mixed form {form}")["out"]
        assert box["took"] == took and np.array_equal(out.reshape(want.shape), want), form


def test_one_1080p_frame_to_the_models_square_and_one_mask_back(lib, ctx):
    frame = _images(3300, 2, (1920, 1080), 3)[1:]                    # the steps
    want = vr.lanczos_resize(frame, (320, 320), 3)
    assert want.min() == 0 and want.max() == 255
    for form in (AUTO, FUSED):
        box = {}

        def down(run):
            _resize_body(lib, ctx, frame, (320, 320), 3, ALIGNED, form)(run)
            box["took"] = run.took
        out = fp.twice(RESIZE, down, seed=form, what=f"1080p form {form}")["out"]
        assert box["took"] == (form or TWO) and np.array_equal(out.reshape(want.shape), want)
    mask = _images(3301, 1, (320, 320), 1)
    want = vr.lanczos_resize(mask, (1920, 1080), 1)

    def up(run):
        _resize_body(lib, ctx, mask, (1920, 1080), 1, ODD, AUTO)(run)
        box["took"] = run.took
    out = fp.twice(RESIZE, up, seed=5, what="mask to 1080p")["out"]
    assert box["took"] == TWO and np.array_equal(out.reshape(want.shape), want)


# ---- mdvt_mask_model_input -----------------------------------------------------------------------------------------------------------
def _input_body(lib, ctx, frames, size, bgr, lays, mean=vr.U2NET_MEAN, std=vr.U2NET_STD):
    L = lib.load()
    N, H, W = frames.shape[:3]
    w, h = size
    lin, lout = lays[0], _f32(lays[1])
    d3 = C.c_double * 3

    def body(run, **wrong):
        ain = run.inp("frames", frames.reshape(N, H, W * 3), lin)
        aout = run.out("out", h, 4 * w, 3 * N, lout)                  # the layout's gap lies between planes
        h_mean, h_std = d3(*mean), d3(*std)
        a = dict(ctx=ctx.handle, in_w=W, in_h=H, n=N, frames=_vp(ain), frames_pitch=ain.pitch, frames_stride=ain.stride, order=int(bgr),
                 model_w=w, model_h=h, mean=C.cast(h_mean, C.c_void_p), std=C.cast(h_std, C.c_void_p), out=_vp(aout), out_pitch=aout.pitch,
                 out_plane_stride=aout.stride, out_stride=3 * aout.stride)
        a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})
        rc = L.mdvt_mask_model_input(a["ctx"], a["in_w"], a["in_h"], a["n"], a["frames"], a["frames_pitch"], a["frames_stride"], a["order"],
                                     a["model_w"], a["model_h"], a["mean"], a["std"], a["out"], a["out_pitch"], a["out_plane_stride"],
                                     a["out_stride"], None)
        if not wrong:
            ctx.check(rc)
        run.vector = fp.all_aligned([aout], 16) and w >= 4
        return rc
    return body


INPUT_CASES = [((1, 1), (320, 320)), ((5, 4), (320, 320)), ((37, 23), (320, 320)), ((333, 187), (320, 320)), ((641, 321), (320, 320)),
               ((320, 200), (320, 320)), ((320, 320), (320, 320)), ((45, 31), (13, 7))]


@pytest.mark.parametrize("case", INPUT_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-to-{c[1][0]}x{c[1][1]}")
def test_model_input_equals_the_restatement_and_keeps_its_footprint(lib, ctx, case):
    src, size = case
    frames = _images(3400 + src[0], 3, src, 3)
    frames[2] //= 3                                                  # a maximum below 255: the division by it shows
    if src == (5, 4):
        frames[1] = 0                                                # an all-zero frame: m = 1e-6
    want = vr.mask_model_input(frames, size)
    assert np.isfinite(want).all() and (src != (5, 4) or np.all(want[1, 0] == F((0.0 / 1e-6 - 0.485) / 0.229)))
    vector = cases = 0
    for k, (lays, N, bgr) in enumerate((lays, N, bgr) for lays in LAYOUTS for N in (1, 3) for bgr in (0, 1)):
        stored = np.ascontiguousarray(frames[:N, ..., ::-1] if bgr else frames[:N])
        box = {}

        def accepted(run):
            _input_body(lib, ctx, stored, size, bgr, lays)(run)
            box["vector"] = run.vector
        tag = f"input {src}->{size} n={N} bgr={bgr} {lays}"
        out = fp.twice(INPUT, accepted, seed=k, what=tag)["out"]
        fp.accepted(INPUT, vector=box["vector"])
        vector, cases = vector + int(box["vector"]), cases + 1
        got = np.ascontiguousarray(out).view(F).reshape(N, 3, size[1], size[0])
        assert np.array_equal(got.view(np.uint32), want[:N].view(np.uint32)), tag
    assert cases - vector >= 4 and (vector >= 4 or size[0] % 4), "both the 16-byte stores and the element stores ran"
    fp.finish_entry(INPUT, need_odd=True, need_padded=True, need_vector=size[0] % 4 == 0)


def test_model_input_takes_other_models_numbers(lib, ctx):
    frames = _images(3450, 2, (40, 30), 3)
    mean, std = (0.5, 0.25, 0.125), (1.0, 0.5, 2.0)
    want = vr.mask_model_input(frames, (17, 11), mean, std)
    out = fp.twice(INPUT, lambda run: _input_body(lib, ctx, frames, (17, 11), 0, ODD, mean, std)(run), seed=1)["out"]
    assert np.array_equal(np.ascontiguousarray(out).view(np.uint32).reshape(2, 3, 11, 17), want.view(np.uint32))


# ---- mdvt_mask_from_prediction -------------------------------------------------------------------------------------------------------
def _mask_body(lib, ctx, pred, size, channels, lays):
    L = lib.load()
    N, ph, pw = pred.shape
    W, H = size
    lin, lout = _f32(lays[0]), lays[1]

    def body(run, **wrong):
        ain = run.inp("pred", pred, lin)
        aout = run.out("mask", H, channels * W, N, lout)
        a = dict(ctx=ctx.handle, pred_w=pw, pred_h=ph, n=N, pred=_vp(ain), pred_pitch=ain.pitch, pred_stride=ain.stride, out_w=W, out_h=H,
                 out_channels=channels, mask=_vp(aout), mask_pitch=aout.pitch, mask_stride=aout.stride)
        a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})
        rc = L.mdvt_mask_from_prediction(a["ctx"], a["pred_w"], a["pred_h"], a["n"], a["pred"], a["pred_pitch"], a["pred_stride"], a["out_w"],
                                         a["out_h"], a["out_channels"], a["mask"], a["mask_pitch"], a["mask_stride"], None)
        if not wrong:
            ctx.check(rc)
        return rc
    return body


def _predictions(seed, n, pw, ph):
    """A sigmoid's range, values outside [0, 1], a tiny range with both zeros."""
    rng = np.random.default_rng(seed)
    pred = rng.normal(0.4, 0.5, (n, ph, pw)).astype(F)
    pred[0] = 1 / (1 + np.exp(-4 * pred[0]))
    if n > 2:
        pred[2] *= F(1e-3)
        pred[2].reshape(-1)[:2] = [-0.0, 0.0]
    return pred


MASK_CASES = [((320, 320), (1, 1)), ((320, 320), (5, 4)), ((320, 320), (37, 23)), ((320, 320), (320, 200)), ((320, 320), (641, 361)),
              ((320, 320), (1000, 7)), ((33, 21), (33, 21)), ((24, 20), (96, 54))]


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-to-{c[1][0]}x{c[1][1]}")
def test_mask_equals_the_restatement_and_keeps_its_footprint(lib, ctx, case):
    (pw, ph), size = case
    pred = _predictions(3500 + size[0], 3, pw, ph)
    want = vr.mask_from_prediction(pred, size)
    assert vr.prediction_bytes(pred).min() == 0 and vr.prediction_bytes(pred).max() == 255
    for k, (lays, N, channels) in enumerate((lays, N, ch) for lays in LAYOUTS for N in (1, 3) for ch in (1, 3)):
        tag = f"mask {pw}x{ph}->{size} n={N} channels={channels} {lays}"
        out = fp.twice(MASK, lambda run: _mask_body(lib, ctx, pred[:N], size, channels, lays)(run), seed=k, what=tag)["mask"]
        fp.accepted(MASK)
        got = out.reshape((N, size[1], size[0]) + ((3,) if channels == 3 else ()))
        if channels == 3:
            assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2]), tag
            got = got[..., 0]
        assert np.array_equal(got, want[:N]), tag
    fp.finish_entry(MASK, need_odd=True, need_padded=True)


def test_mask_decrees_a_constant_or_non_finite_plane_is_all_zero(lib, ctx):
    rng = np.random.default_rng(3600)
    pred = rng.normal(0.5, 0.3, (6, 20, 24)).astype(F)
    pred[1] = F(0.75)                                                # ma == mi
    pred[2, 7, 9] = np.nan
    pred[3, 0, 0] = np.inf
    pred[4, 19, 23] = -np.inf
    pred[5, 3, :2] = [-3e38, 3e38]                                   # fl(ma - mi) is infinite
    want = vr.mask_from_prediction(pred, (50, 30))
    assert want[0].any() and not want[1:].any()
    for size in ((50, 30), (24, 20)):
        want = vr.mask_from_prediction(pred, size)
        for channels in (1, 3):
            out = fp.twice(MASK, lambda run: _mask_body(lib, ctx, pred, size, channels, ODD)(run), seed=channels)["mask"]
            got = out.reshape((6, size[1], size[0]) + ((3,) if channels == 3 else ()))
            assert np.array_equal(got if channels == 1 else got[..., 2], want) and not got[1:].any()


def test_one_mask_to_1080p(lib, ctx):
    pred = _predictions(3700, 1, 320, 320)
    want = vr.mask_from_prediction(pred, (1920, 1080), channels=3)
    out = fp.twice(MASK, lambda run: _mask_body(lib, ctx, pred, (1920, 1080), 3, ALIGNED)(run), seed=1)["mask"]
    assert np.array_equal(out.reshape(want.shape), want)


# ---- launch sets --------------------------------------------------------------------------------------------------------------------
def test_all_three_run_in_launch_sets_under_a_small_workspace(lib, tool):
    """workspace_mib = 1: eight frames do not fit one launch set of any of the three calls (the two-launch form's intermediate image
    of 187 x 320 x 3 bytes: 5 frames; the model's 320 x 320 x 3 image with its 321 x 320 x 3 intermediate: 1; a 320 x 320 byte plane
    with its 320 x 641 intermediate: 3)."""
    import torch
    ctx = gc.make_context(lib, 16, 16, workspace_mib=1)
    try:
        frames = _images(3900, 8, (333, 187), 3)
        got, took = tool.lanczos_resize(ctx, torch.from_numpy(frames).cuda(), (320, 320))
        assert took == TWO and np.array_equal(got.cpu().numpy(), vr.lanczos_resize(frames, (320, 320), 3))
        assert ctx.workspace_bytes() < 8 * 187 * 320 * 3
        frames = _images(3901, 8, (641, 321), 3)
        x = tool.mask_model_input(ctx, torch.from_numpy(frames).cuda(), (320, 320), vr.U2NET_MEAN, vr.U2NET_STD)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), vr.mask_model_input(frames).view(np.uint32))
        pred = _predictions(3902, 8, 320, 320)
        mask = tool.mask_from_prediction(ctx, torch.from_numpy(pred).cuda(), (641, 361), channels=1)
        assert np.array_equal(mask.cpu().numpy(), vr.mask_from_prediction(pred, (641, 361)))
        assert ctx.workspace_bytes() < 2 << 20
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


def test_resize_refusals_leave_their_text_and_write_nothing(lib, ctx):
    N, (W, H), (w, h) = 2, (9, 5), (12, 7)
    none = C.c_void_p(None)
    for ch in (1, 3):
        images = _images(3800, N, (W, H), ch)
        body = _resize_body(lib, ctx, images, (w, h), ch, ALIGNED, AUTO)
        big = dict(in_pitch=1 << 16, in_stride=1 << 32, out_pitch=1 << 16, out_stride=1 << 32)
        cases = [("NULL in", dict(d_in=none), INVALID, "NULL buffer"), ("NULL out", dict(d_out=none), INVALID, "NULL buffer"),
                 ("in_w 0", dict(in_w=0), INVALID, "bad size"), ("in_h -1", dict(in_h=-1), INVALID, "bad size"),
                 ("out_w 0", dict(out_w=0), INVALID, "bad size"), ("out_h 0", dict(out_h=0), INVALID, "bad size"),
                 ("channels 2", dict(channels=2), INVALID, "channels must be 1 or 3"), ("channels 4", dict(channels=4), INVALID, "channels must be 1 or 3"),
                 ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"),
                 ("form 3", dict(form=3), INVALID, "form must be"), ("form -1", dict(form=-1), INVALID, "form must be"),
                 ("a short in pitch", dict(in_pitch=ch * W - 1), INVALID, "in_pitch smaller than one row"),
                 ("a short out pitch", dict(out_pitch=ch * w - 1), INVALID, "out_pitch smaller than one row"),
                 ("a short in stride", dict(in_stride=ch * W * H - 1), INVALID, "stride smaller than one frame"),
                 ("a short out stride", dict(out_stride=ch * w * h - 1), INVALID, "stride smaller than one frame"),
                 ("in_w 8193", dict(in_w=8193, **big), UNSUPPORTED, "size beyond 8192"), ("in_h 8193", dict(in_h=8193, **big), UNSUPPORTED, "size beyond 8192"),
                 ("out_w 8193", dict(out_w=8193, **big), UNSUPPORTED, "size beyond 8192"), ("out_h 8193", dict(out_h=8193, **big), UNSUPPORTED, "size beyond 8192"),
                 ("fused with one pass", dict(form=FUSED, out_w=W, out_pitch=ch * W, out_stride=ch * W * h), UNSUPPORTED, "the fused form needs both passes")]
        _refused(lib, ctx, RESIZE, body, cases)
        fp.twice(RESIZE, lambda run: body(run), seed=99)            # the context still works after them


def test_model_input_refusals_leave_their_text_and_write_nothing(lib, ctx):
    N, (W, H), (w, h) = 2, (9, 5), (12, 7)
    frames = _images(3801, N, (W, H), 3)
    none = C.c_void_p(None)
    d3 = C.c_double * 3
    keep = [d3(0.5, float("nan"), 0.5), d3(1.0, 0.0, 1.0), d3(1.0, float("inf"), 1.0)]
    body = _input_body(lib, ctx, frames, (w, h), 0, ALIGNED)
    big = dict(frames_pitch=1 << 16, frames_stride=1 << 32, out_pitch=1 << 16, out_plane_stride=1 << 32, out_stride=3 << 32)
    cases = [("NULL frames", dict(frames=none), INVALID, "NULL buffer"), ("NULL out", dict(out=none), INVALID, "NULL buffer"),
             ("NULL mean", dict(mean=none), INVALID, "NULL mean or std"), ("NULL std", dict(std=none), INVALID, "NULL mean or std"),
             ("in_w 0", dict(in_w=0), INVALID, "bad size"), ("in_h 0", dict(in_h=0), INVALID, "bad size"),
             ("model_w 0", dict(model_w=0), INVALID, "bad size"), ("model_h -1", dict(model_h=-1), INVALID, "bad size"),
             ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"), ("order 2", dict(order=2), INVALID, "order must be"),
             ("a NaN mean", dict(mean=C.cast(keep[0], C.c_void_p)), INVALID, "mean must be finite"),
             ("a std of 0", dict(std=C.cast(keep[1], C.c_void_p)), INVALID, "mean must be finite"),
             ("an infinite std", dict(std=C.cast(keep[2], C.c_void_p)), INVALID, "mean must be finite"),
             ("a short frames pitch", dict(frames_pitch=3 * W - 1), INVALID, "frames_pitch smaller than one row"),
             ("a short out pitch", dict(out_pitch=4 * w - 4), INVALID, "out_pitch smaller than one row"),
             ("a short plane stride", dict(out_plane_stride=4 * w * h - 4), INVALID, "out_plane_stride smaller than one plane"),
             ("a short frames stride", dict(frames_stride=3 * W * H - 1), INVALID, "stride smaller than one frame"),
             ("a short out stride", dict(out_stride=12 * w * h - 4), INVALID, "stride smaller than one frame"),
             ("an out pitch of 4 w + 1", dict(out_pitch=4 * w + 1, out_plane_stride=(4 * w + 4) * h, out_stride=3 * (4 * w + 4) * h), INVALID, "must be multiples of 4"),
             ("a plane stride off by 2", dict(out_plane_stride=4 * w * h + 2, out_stride=3 * (4 * w * h + 4)), INVALID, "must be multiples of 4"),
             ("an out stride off by 1", dict(out_stride=12 * w * h + 1), INVALID, "must be multiples of 4"),
             ("d_out off by 1", dict(out=_moved("out", 1)), INVALID, "must be multiples of 4"),
             ("in_w 8193", dict(in_w=8193, **big), UNSUPPORTED, "size beyond 8192"), ("model_h 8193", dict(model_h=8193, **big), UNSUPPORTED, "size beyond 8192")]
    _refused(lib, ctx, INPUT, body, cases)
    fp.twice(INPUT, lambda run: body(run), seed=99)


def test_mask_refusals_leave_their_text_and_write_nothing(lib, ctx):
    N, (pw, ph), (W, H) = 2, (9, 5), (12, 7)
    pred = _predictions(3802, N, pw, ph)
    none = C.c_void_p(None)
    for channels in (1, 3):
        body = _mask_body(lib, ctx, pred, (W, H), channels, ALIGNED)
        big = dict(pred_pitch=1 << 16, pred_stride=1 << 32, mask_pitch=1 << 16, mask_stride=1 << 32)
        cases = [("NULL pred", dict(pred=none), INVALID, "NULL buffer"), ("NULL mask", dict(mask=none), INVALID, "NULL buffer"),
                 ("pred_w 0", dict(pred_w=0), INVALID, "bad size"), ("pred_h 0", dict(pred_h=0), INVALID, "bad size"),
                 ("out_w -1", dict(out_w=-1), INVALID, "bad size"), ("out_h 0", dict(out_h=0), INVALID, "bad size"),
                 ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"),
                 ("out_channels 2", dict(out_channels=2), INVALID, "out_channels must be 1 or 3"), ("out_channels 0", dict(out_channels=0), INVALID, "out_channels must be 1 or 3"),
                 ("a short pred pitch", dict(pred_pitch=4 * pw - 4), INVALID, "pred_pitch smaller than one row"),
                 ("a short mask pitch", dict(mask_pitch=channels * W - 1), INVALID, "mask_pitch smaller than one row"),
                 ("a short pred stride", dict(pred_stride=4 * pw * ph - 4), INVALID, "stride smaller than one frame"),
                 ("a short mask stride", dict(mask_stride=channels * W * H - 1), INVALID, "stride smaller than one frame"),
                 ("a pred pitch of 4 w + 2", dict(pred_pitch=4 * pw + 2, pred_stride=(4 * pw + 4) * ph), INVALID, "must be multiples of 4"),
                 ("a pred stride off by 2", dict(pred_stride=4 * pw * ph + 2), INVALID, "must be multiples of 4"),
                 ("d_pred off by 1", dict(pred=_moved("pred", 1)), INVALID, "must be multiples of 4"),
                 ("pred_w 8193", dict(pred_w=8193, **big), UNSUPPORTED, "size beyond 8192"), ("out_h 8193", dict(out_h=8193, **big), UNSUPPORTED, "size beyond 8192")]
        _refused(lib, ctx, MASK, body, cases)
        fp.twice(MASK, lambda run: body(run), seed=99)
