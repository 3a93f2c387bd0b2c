"""The four entry points of include/mdvt_megasam.h through the raw C ABI, bit for bit against tests/megasam_ref.py (NumPy on the test
machine), in the arenas of tests/footprint.py -- every output in poison, each case run on a poison and on its complement, so nothing
outside an output's payload changes, every payload byte is written and no byte behind an input row's end matters -- with aligned
layouts (the 16-byte loads and stores), padded pitches, gapped strides and odd bases (the byte and element paths).  Every refusal
leaves its text and writes nothing."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import megasam_ref as gr
import metric_align_ref as mr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
F = np.float32
AREA, DEPTH, MASK, OUTPUTS = "mdvt_area_model_frames", "mdvt_tracker_depth", "mdvt_tracker_mask", "mdvt_tracker_outputs"

# (in_w, in_h), (mid_w, mid_h), (out_w, out_h): the issue's two small cases
SMALL = [((37, 29), (11, 9), (8, 8)), ((59, 33), (18, 10), (16, 8))]

# layouts (packed bytes, float planes): float planes in bytes, kept multiples of 4 (a float32 lies at its alignment)
ALIGNED = (fp.Layout(0, 0, 0), fp.Layout(0, 0, 0))                      # tight
PADDED16 = (fp.Layout(0, 5 + 16 * 3, 32), fp.Layout(0, 16, 32))         # padded pitches, gapped strides (made multiples of 16 per case below)
ODD = (fp.Layout(1, 3, 5), fp.Layout(4, 12, 20))                        # odd bases: the byte and element paths
LAYOUTS = (ALIGNED, PADDED16, ODD)


def _vp(a):
    return C.c_void_p(a.ptr)


def _bytes_layout(lay, row_bytes, rows):
    """PADDED16 for packed bytes: a padding and a gap that make this case's pitch and stride multiples of 16, both non-zero."""
    if lay is not PADDED16[0]:
        return lay
    pad = 16 + (-row_bytes) % 16
    return fp.Layout(0, pad, 32 + (-(rows * (row_bytes + pad))) % 16)


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
    for e in (AREA, DEPTH, MASK, OUTPUTS):
        fp.TALLY.pop(e, None)                          # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def _error(lib, ctx):
    return (lib.load().mdvt_last_error(ctx.handle) or b"").decode()


# ---- mdvt_area_model_frames ---------------------------------------------------------------------------------------------------------
def _area_body(lib, ctx, frames, mid, out, bgr, lays, box=None):
    L = lib.load()
    N, H, W = frames.shape[:3]
    (w1, h1), (wc, hc) = mid, out

    def body(run, **wrong):
        ain = run.inp("frames", frames, _bytes_layout(lays[0], 3 * W, H))
        aout = run.out("out", 3 * hc, wc, N, _bytes_layout(lays[0], wc, 3 * hc))
        a = dict(in_w=W, in_h=H, n=N, frames=_vp(ain), frames_pitch=ain.pitch, frames_stride=ain.stride, bgr=int(bgr), mid_w=w1, mid_h=h1,
                 out_w=wc, out_h=hc, out=_vp(aout), out_pitch=aout.pitch, out_plane_stride=hc * aout.pitch, out_stride=aout.stride)
        a.update(wrong)
        rc = L.mdvt_area_model_frames(ctx.handle, a["in_w"], a["in_h"], a["n"], a["frames"], a["frames_pitch"], a["frames_stride"], a["bgr"],
                                      a["mid_w"], a["mid_h"], a["out_w"], a["out_h"], a["out"], a["out_pitch"], a["out_plane_stride"],
                                      a["out_stride"], None)
        if not wrong:
            ctx.check(rc)
        if box is not None:
            box["vector"] = L.mdvt_megasam_vector_path(W, N, _vp(ain), ain.pitch, ain.stride)
            box["text"] = _error(lib, ctx)
        return rc
    return body


def _pixels(rng, N, H, W):
    rgb = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    rgb[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 1], [1, 254, 255]]
    rgb[-1, H // 2:] = 255                                          # a white block: sums at the upper clamp
    return rgb


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_area_frames_equal_the_restatement_and_keep_their_footprint(lib, ctx, case):
    (W, H), mid, out = case
    rgb = _pixels(np.random.default_rng(2600 + W), 3, H, W)
    want = gr.area_model_frames(rgb, mid, out)                      # computed once, shared
    vector = cases = 0
    for k, (lays, N, bgr) in enumerate((lays, N, bgr) for lays in LAYOUTS for N in (1, 3) for bgr in (0, 1)):
        stored = np.ascontiguousarray(rgb[:N, ..., ::-1] if bgr else rgb[:N])
        box = {}
        tag = f"{N}x{W}x{H}->{mid}->{out} bgr={bgr} {lays}"
        got = fp.twice(AREA, _area_body(lib, ctx, stored, mid, out, bgr, lays, box), seed=k, what=tag)["out"]
        fp.accepted(AREA, vector=bool(box["vector"]))
        assert box["vector"] == int(lays is PADDED16), tag          # a base, a pitch and a stride that are multiples of 16 take the 16-byte loads
        vector, cases = vector + box["vector"], cases + 1
        assert np.array_equal(got.reshape(N, 3, out[1], out[0]), want[:N]), tag
    assert vector >= 4 and cases - vector >= 4, "both the 16-byte loads and the byte path ran"
    fp.finish_entry(AREA, need_odd=True, need_padded=True, need_vector=True)


def test_area_widths_on_either_side_of_a_16_byte_row_and_equal_sizes(lib, ctx):
    """A row of 5 pixels is 15 bytes, of 6 pixels 18: the smallest rows without and with a whole 16-byte load, asserted through the
    path query.  Equal sizes are a crop into planes; one equal axis leaves that axis alone."""
    for (W, H), mid, out, vec in (((5, 7), (3, 4), (3, 4), 0), ((6, 7), (4, 5), (4, 4), 1), ((21, 7), (13, 5), (8, 5), 1),
                                  ((9, 7), (9, 7), (8, 6), 1), ((9, 7), (9, 4), (9, 4), 1), ((9, 7), (5, 7), (5, 7), 1)):
        rgb = _pixels(np.random.default_rng(2620 + W), 2, H, W)
        box = {}
        got = fp.twice(AREA, _area_body(lib, ctx, rgb, mid, out, 0, PADDED16, box), what=f"{W}x{H}")["out"]
        assert box["vector"] == vec, (W, H)
        assert np.array_equal(got.reshape(2, 3, out[1], out[0]), gr.area_model_frames(rgb, mid, out)), (W, H, mid)
        if (W, H) == mid:
            assert np.array_equal(got.reshape(2, 3, out[1], out[0]), rgb[:, :out[1], :out[0]].transpose(0, 3, 1, 2))


def test_area_of_a_full_size_frame(lib, ctx):
    """1920 x 1080 -> 591 x 332 -> 584 x 328, the tracker's size for every 16:9 video: three column tiles, up to 5 x 5 taps."""
    rgb = _pixels(np.random.default_rng(2630), 1, 1080, 1920)
    box = {}
    got = fp.twice(AREA, _area_body(lib, ctx, rgb, (591, 332), (584, 328), 0, ALIGNED, box), what="1080p")["out"]
    assert box["vector"] == 1
    assert np.array_equal(got.reshape(1, 3, 328, 584), gr.area_model_frames(rgb, (591, 332), (584, 328)))


def test_area_refusals_name_their_reason_and_write_nothing(lib, ctx):
    rgb = _pixels(np.random.default_rng(2640), 2, 12, 8)
    for wrong, status, text in ((dict(mid_w=4, mid_h=6), UNSUPPORTED, "integer factors 2 x 2"),
                                (dict(mid_w=2, mid_h=4, out_w=2, out_h=4), UNSUPPORTED, "integer factors 4 x 3"),
                                (dict(mid_w=9, mid_h=12), UNSUPPORTED, "area enlargement is another algorithm"),
                                (dict(mid_w=5, mid_h=13, out_w=4, out_h=4), UNSUPPORTED, "area enlargement is another algorithm"),
                                (dict(out_w=6), INVALID, "larger than the resized image"),
                                (dict(bgr=2), INVALID, "bgr must be 0"),
                                (dict(n=0), INVALID, "n_frames"),
                                (dict(frames_pitch=23), INVALID, "frames_pitch smaller than one row"),
                                (dict(out_pitch=3), INVALID, "out_pitch smaller than one row"),
                                (dict(out_plane_stride=4), INVALID, "out_plane_stride smaller than one plane"),
                                (dict(frames_stride=8), INVALID, "stride smaller than one frame"),
                                (dict(frames=None), INVALID, "NULL buffer")):
        box = {}
        body = _area_body(lib, ctx, rgb, (5, 7), (4, 4), 0, ALIGNED, box)
        fp.refused(AREA, lambda run: body(run, **wrong), status)
        assert text in box["text"], (wrong, box["text"])


# ---- mdvt_tracker_depth, mdvt_tracker_mask --------------------------------------------------------------------------------------------
def _plane_body(lib, ctx, entry, frames, mid, out, bgr, lays, max_depth=None, box=None):
    L = lib.load()
    N, H, W = frames.shape[:3]
    (w1, h1), (wc, hc) = mid, out

    def body(run, **wrong):
        ain = run.inp("frames", frames, _bytes_layout(lays[0], 3 * W, H))
        aout = run.out("out", hc, 4 * wc, N, lays[1])
        a = dict(in_w=W, in_h=H, n=N, frames=_vp(ain), frames_pitch=ain.pitch, frames_stride=ain.stride, bgr=int(bgr), max_depth=max_depth,
                 mid_w=w1, mid_h=h1, out_w=wc, out_h=hc, out=_vp(aout), out_pitch=aout.pitch, out_stride=aout.stride)
        a.update(wrong)
        head = (ctx.handle, a["in_w"], a["in_h"], a["n"], a["frames"], a["frames_pitch"], a["frames_stride"], a["bgr"])
        tail = (a["mid_w"], a["mid_h"], a["out_w"], a["out_h"], a["out"], a["out_pitch"], a["out_stride"], None)
        rc = L.mdvt_tracker_depth(*head, float(a["max_depth"]), *tail) if entry == DEPTH else L.mdvt_tracker_mask(*head, *tail)
        if not wrong:
            ctx.check(rc)
        if box is not None:
            box["vector"] = fp.all_aligned([aout], 16) and wc >= 4
            box["text"] = _error(lib, ctx)
        return rc
    return body


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_tracker_depth_equals_the_restatement_and_keeps_its_footprint(lib, ctx, case):
    (W, H), mid, out = case
    rng = np.random.default_rng(2650 + W)
    rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    rgb[0, :2] = 0                                                  # codes 0 and 255, and mixed bytes everywhere else
    rgb[0, 2:4] = 255
    rgb[1, ..., 1] = 255 - rgb[1, ..., 0]                           # a green byte that differs from red: it is not read
    for max_depth in (100, 20):
        want = gr.tracker_depth(rgb, max_depth, mid, out)
        green = rgb.copy()
        green[..., 1] ^= 0x5A
        assert np.array_equal(gr.tracker_depth(green, max_depth, mid, out), want)
        for k, (lays, N, bgr) in enumerate((lays, N, bgr) for lays in LAYOUTS for N in (1, 3) for bgr in (0, 1)):
            src = green if k % 2 else rgb
            stored = np.ascontiguousarray(src[:N, ..., ::-1] if bgr else src[:N])
            box = {}
            tag = f"{N}x{W}x{H}->{mid}->{out} bgr={bgr} max_depth={max_depth} {lays}"
            got = fp.twice(DEPTH, _plane_body(lib, ctx, DEPTH, stored, mid, out, bgr, lays, max_depth, box), seed=k, what=tag)["out"]
            fp.accepted(DEPTH, vector=box["vector"])
            assert mr.same_bits(got.view(F).reshape(N, out[1], out[0]), want[:N]).size == 0, tag
    assert float(want.min()) == 0.0 and float(want.max()) > 20.0           # 0xFFFF0000 lies above 255^4: the largest code decodes above max_depth
    fp.finish_entry(DEPTH, need_odd=True, need_padded=True, need_vector=True)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_tracker_mask_equals_the_restatement_and_keeps_its_footprint(lib, ctx, case):
    (W, H), mid, out = case
    rng = np.random.default_rng(2670 + W)
    ramp = np.broadcast_to((np.arange(W) * 255 // (W - 1)).astype(np.uint8)[None, :, None], (H, W, 3))
    frames = np.stack([np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), ramp, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)])
    want = gr.tracker_mask(frames, mid, out)                        # black, white, a grey ramp and coloured noise
    assert float(np.abs(want[0] - 1).max()) < 1e-6 and np.all(want[1] == 0)
    for k, (lays, bgr) in enumerate((lays, bgr) for lays in LAYOUTS for bgr in (0, 1)):
        for first, N in ((0, 4), (3, 1)):
            stored = np.ascontiguousarray(frames[first:first + N, ..., ::-1] if bgr else frames[first:first + N])
            box = {}
            tag = f"{N}x{W}x{H}->{mid}->{out} bgr={bgr} {lays}"
            got = fp.twice(MASK, _plane_body(lib, ctx, MASK, stored, mid, out, bgr, lays, box=box), seed=k, what=tag)["out"]
            fp.accepted(MASK, vector=box["vector"])
            assert mr.same_bits(got.view(F).reshape(N, out[1], out[0]), want[first:first + N]).size == 0, tag
    fp.finish_entry(MASK, need_odd=True, need_padded=True, need_vector=True)


def test_tracker_mask_above_torchs_kernel_switch(lib, ctx):
    """mid_w + mid_h > 128: the two-pass form of the bilinear sum."""
    rgb = np.random.default_rng(2680).integers(0, 256, (1, 54, 240, 3), dtype=np.uint8)
    got = fp.twice(MASK, _plane_body(lib, ctx, MASK, rgb, (121, 27), (120, 24), 0, ALIGNED), what="two-pass")["out"]
    assert mr.same_bits(got.view(F).reshape(1, 24, 120), gr.tracker_mask(rgb, (121, 27), (120, 24))).size == 0


def test_tracker_plane_refusals_name_their_reason_and_write_nothing(lib, ctx):
    rgb = np.zeros((2, 12, 8, 3), np.uint8)
    for entry in (DEPTH, MASK):
        cases = [(dict(out_h=8), INVALID, "larger than the resized image"), (dict(bgr=-1), INVALID, "bgr must be 0"),
                 (dict(out_pitch=12), INVALID, "out_pitch smaller than one row"), (dict(out_stride=16), INVALID, "stride smaller than one frame"),
                 (dict(out_pitch=18, out_stride=80), INVALID, "multiples of 4"), (dict(mid_w=0), INVALID, "bad size")]
        if entry == DEPTH:
            cases += [(dict(max_depth=0.0), INVALID, "max_depth must be > 0"), (dict(max_depth=float("nan")), INVALID, "max_depth must be > 0")]
        for wrong, status, text in cases:
            box = {}
            body = _plane_body(lib, ctx, entry, rgb, (5, 7), (4, 4), 0, ALIGNED, 100, box)
            fp.refused(entry, lambda run: body(run, **wrong), status)
            assert text in box["text"], (entry, wrong, box["text"])


# ---- mdvt_tracker_outputs -------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([np.nan, np.inf, 3.5, -np.inf, 0.25, -1.5, -0.0, 0.0, 1e-40, 250.0, 0.99999994, 1.0, 20.0, 100.0, 0.5], F)


def _planes(rng, N, h, w, top):
    x = (rng.random((N, h, w), dtype=F) * F(1.3 * top) - F(0.1 * top)).astype(F)
    flat = x.reshape(-1)
    flat[::5] = np.resize(SPECIALS, flat[::5].size)
    return x


def _outputs_body(lib, ctx, planes, mode, max_value, out_size, bgr, lays, box=None):
    L = lib.load()
    N, h, w = planes.shape
    W, H = out_size

    def body(run, **wrong):
        ain = run.inp("planes", planes, lays[1])
        aout = run.out("frames", H, 3 * W, N, lays[0] if lays[0] is not PADDED16[0] else fp.Layout(0, 4 + (-3 * W) % 4, 8))
        a = dict(mode=mode, in_w=w, in_h=h, n=N, planes=_vp(ain), planes_pitch=ain.pitch, planes_stride=ain.stride, max_value=float(max_value),
                 out_w=W, out_h=H, frames=_vp(aout), frames_pitch=aout.pitch, frames_stride=aout.stride, bgr=int(bgr))
        a.update(wrong)
        rc = L.mdvt_tracker_outputs(ctx.handle, a["mode"], a["in_w"], a["in_h"], a["n"], a["planes"], a["planes_pitch"], a["planes_stride"],
                                    a["max_value"], a["out_w"], a["out_h"], a["frames"], a["frames_pitch"], a["frames_stride"], a["bgr"], None)
        if not wrong:
            ctx.check(rc)
        if box is not None:
            box["vector"] = fp.all_aligned([aout], 4) and W >= 4
            box["text"] = _error(lib, ctx)
        return rc
    return body


@pytest.mark.parametrize("mode", [0, 1], ids=["depth_video", "grey_video"])
def test_tracker_outputs_equal_the_restatement_and_keep_their_footprint(lib, ctx, mode):
    """Mode 0 with values below 0, above max_depth, NaN and both infinities (the sink's rules); mode 1 with values below 0, above 1 and
    NaN; both resized (9 x 11 -> 37 x 29) and at equal size."""
    top = 20.0 if mode == 0 else 1.0
    for s, ((w, h), (W, H)) in enumerate((((9, 11), (37, 29)), ((37, 29), (37, 29)), ((12, 7), (12, 7)), ((40, 23), (16, 9)))):
        x = _planes(np.random.default_rng(2700 + 10 * mode + s), 3, h, w, top)
        for bgr in (0, 1):
            want = gr.tracker_outputs(x, mode, top, (W, H), bool(bgr))
            for k, (lays, N) in enumerate((lays, N) for lays in LAYOUTS for N in (1, 3)):
                box = {}
                tag = f"mode {mode} {N}x{w}x{h}->{W}x{H} bgr={bgr} {lays}"
                got = fp.twice(OUTPUTS, _outputs_body(lib, ctx, x[:N], mode, top, (W, H), bgr, lays, box), seed=k, what=tag)["frames"]
                fp.accepted(OUTPUTS, vector=box["vector"])
                assert np.array_equal(got.reshape(N, H, W, 3), want[:N]), tag
    fp.finish_entry(OUTPUTS, need_odd=True, need_padded=True, need_vector=True)


def test_tracker_outputs_refusals_name_their_reason_and_write_nothing(lib, ctx):
    x = np.zeros((2, 8, 12), F)
    for mode, wrong, status, text in ((1, dict(out_w=6, out_h=4), UNSUPPORTED, "an exact 2 x reduction"), (2, {"n": 2}, INVALID, "mode must be 0"),
                                      (0, dict(max_value=0.0), INVALID, "max_value must be > 0"), (1, dict(bgr=3), INVALID, "bgr must be 0"),
                                      (0, dict(planes_pitch=44), INVALID, "planes_pitch smaller than one row"),
                                      (0, dict(planes_pitch=50, planes_stride=400), INVALID, "multiples of 4"),
                                      (1, dict(frames_pitch=20), INVALID, "frames_pitch smaller than one row"),
                                      (0, dict(frames_stride=24), INVALID, "stride smaller than one frame")):
        box = {}
        body = _outputs_body(lib, ctx, x, mode, 1.0, (9, 5), 0, ALIGNED, box)
        fp.refused(OUTPUTS, lambda run: body(run, **wrong), status)
        assert text in box["text"], (mode, wrong, box["text"])
    # the depth video takes the 2 x reduction: nearest-exact has no such path
    got = fp.twice(OUTPUTS, _outputs_body(lib, ctx, x + F(3), 0, 100.0, (6, 4), 0, ALIGNED), what="2x nearest")["frames"]
    assert np.array_equal(got.reshape(2, 4, 6, 3), gr.tracker_outputs(x + F(3), 0, 100.0, (6, 4)))
