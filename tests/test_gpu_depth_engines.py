"""The three entry points of include/mdvt_depth_engines.h through the raw C ABI, bit for bit against tests/depth_engines_ref.py (NumPy on
the test machine): mdvt_model_frames and mdvt_depth_prompt in the arenas of tests/footprint.py -- every output in poison, each case
run on a poison and on its complement, so nothing outside the first out_w elements of a row changes, every one of those is written
and no byte behind an input row's end matters -- with aligned layouts (the vector loads and stores), padded pitches, gapped strides
and bases one byte off (the element paths); mdvt_focal_from_points on selections of 0 .. 9216 values around a chunk's edge, both
layouts, special values and launch sets; every refusal, which leaves its text and writes nothing."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import depth_engines_ref as er
import footprint as fp
import geometry_cases as gc
import metric_align_ref as mr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
F = np.float32
FRAMES, PROMPT, FOCAL = "mdvt_model_frames", "mdvt_depth_prompt", "mdvt_focal_from_points"


def _vp(a):
    return C.c_void_p(a.ptr)


def _moved(name, by):
    """The argument `name`, a pointer, `by` bytes further on."""
    return lambda a: C.c_void_p(a[name].value + by)


@pytest.fixture(scope="module")
def lib():
    """The binding.  The arenas are torch tensors: torch opens the device before the library's context does, as in the rest of the
    suite (a module-scoped fixture is set up before any function-scoped one, so the order is settled here)."""
    import torch
    torch.cuda.init()
    from metric_depth_video_toolbox_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0, 16, 16)
    yield c
    c.close()
    for e in (FRAMES, PROMPT, FOCAL):
        fp.TALLY.pop(e, None)                          # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("depth_engine_video_tool", os.path.join(REPO, "tools", "depth_engine_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# layouts: (input, output, gap between the planes of a frame rather than between frames)
ALIGNED = (fp.Layout(0, 0, 0), fp.Layout(0, 0, 0))                      # tight: every vector path where the width allows
PADDED16 = (fp.Layout(4, 8, 12), fp.Layout(0, 16, 32))                  # padded pitches, gapped strides, still multiples of 4 / 16
ODD = (fp.Layout(1, 3, 5), fp.Layout(1, 3, 5))                          # one byte off: the element paths (float planes: 4 off)


# ---- mdvt_model_frames ------------------------------------------------------------------------------------------------------------
def _frames_body(lib, ctx, frames, out_size, fmt, bgr, lays, plane_gap):
    """frames [N, H, W, 3] as stored.  The output arena holds [N, 3, h, w]: plane_gap puts the layout's gap between planes (frames
    then follow at 3 plane strides), else between frames (planes tight)."""
    L = lib.load()
    N, H, W = frames.shape[:3]
    w, h = out_size
    e = 4 if fmt else 1
    lin, lout = lays
    if fmt:
        lout = fp.Layout(lout.base * 4 % 16, lout.pad * 4 if lout.pad % 4 else lout.pad, lout.gap * 4 if lout.gap % 4 else lout.gap)

    def body(run, **wrong):
        ain = run.inp("frames", frames, lin)
        if plane_gap:
            aout = run.out("out", h, e * w, 3 * N, lout)
            pitch, plane, stride = aout.pitch, aout.stride, 3 * aout.stride
        else:
            aout = run.out("out", 3 * h, e * w, N, lout)
            pitch, plane, stride = aout.pitch, h * aout.pitch, aout.stride
        a = dict(ctx=ctx.handle, in_w=W, in_h=H, n=N, frames=_vp(ain), frames_pitch=ain.pitch, frames_stride=ain.stride, order=int(bgr),
                 out_w=w, out_h=h, format=fmt, out=_vp(aout), out_pitch=pitch, out_plane_stride=plane, out_stride=stride)
        a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})      # (a callable makes its wrong value from the right ones)
        rc = L.mdvt_model_frames(a["ctx"], a["in_w"], a["in_h"], a["n"], a["frames"], a["frames_pitch"], a["frames_stride"], a["order"],
                                 a["out_w"], a["out_h"], a["format"], a["out"], a["out_pitch"], a["out_plane_stride"], a["out_stride"], None)
        if not wrong:
            ctx.check(rc)
        run.vector = fp.all_aligned([aout], 16 if fmt else 4) and w >= 4
        return rc
    return body


MODEL_SIZES = {
    "identity": [((13, 5), (13, 5)), ((16, 9), (16, 9)), ((17, 9), (17, 9)), ((16, 5), (16, 5))],
    "up_to_a_multiple_of_14": [((17, 9), (28, 14)), ((13, 5), (14, 14)), ((16, 9), (28, 14))],
    "down_not_2x": [((17, 9), (13, 5)), ((16, 9), (13, 5)), ((17, 9), (16, 5))],
    "down_exactly_2x": [((26, 10), (13, 5)), ((32, 18), (16, 9)), ((34, 18), (17, 9))],
}


@pytest.mark.parametrize("kind", sorted(MODEL_SIZES))
def test_model_frames_equal_the_restatement_and_keep_their_footprint(lib, ctx, kind):
    vector = cases = 0
    for s, ((W, H), (w, h)) in enumerate(MODEL_SIZES[kind]):
        rng = np.random.default_rng(1800 + 10 * sorted(MODEL_SIZES).index(kind) + s)
        rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        rgb[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 1], [1, 254, 255]]
        want = {False: er.model_frames(rgb, (w, h)), True: er.model_frames(rgb, (w, h), as_float=True)}     # computed once, shared
        for k, (lays, N, bgr, fmt) in enumerate((lays, N, bgr, fmt) for lays in (ALIGNED, PADDED16, ODD) for N in (1, 3) for bgr in (0, 1)
                                                for fmt in (0, 1)):
            stored = np.ascontiguousarray(rgb[:N, ..., ::-1] if bgr else rgb[:N])
            body = _frames_body(lib, ctx, stored, (w, h), fmt, bgr, lays, plane_gap=k % 2 == 0)
            box = {}

            def accepted(run):
                body(run)
                box["vector"] = run.vector
            tag = f"{kind} {N}x{W}x{H}->{w}x{h} bgr={bgr} fmt={fmt} {lays}"
            out = fp.twice(FRAMES, accepted, seed=k, what=tag)["out"]
            fp.accepted(FRAMES, vector=box["vector"])
            vector, cases = vector + int(box["vector"]), cases + 1
            if fmt:
                got = np.ascontiguousarray(out).view(F).reshape(N, 3, h, w)
                assert mr.same_bits(got, want[True][:N]).size == 0, tag
            else:
                assert np.array_equal(out.reshape(N, 3, h, w), want[False][:N]), tag
    assert vector >= 4 and cases - vector >= 4, "both the vector stores and the element path ran"
    fp.finish_entry(FRAMES, need_odd=True, need_padded=True, need_vector=True)


def test_model_frames_float_is_one_division_on_all_256_values(lib, ctx, tool):
    import torch
    v = np.arange(256, dtype=np.uint8)
    frames = np.stack([v, v[::-1], np.roll(v, 7)], axis=-1).reshape(1, 16, 16, 3)
    got = tool.model_frames(ctx, torch.from_numpy(frames).cuda(), as_float=True).cpu().numpy()
    assert mr.same_bits(got[0, 0].ravel(), v.astype(F) / F(255)).size == 0
    assert mr.same_bits(got, er.model_frames(frames, as_float=True)).size == 0
    assert np.any(got[0, 0].ravel() != v.astype(F) * F(1.0 / 255.0))


def test_model_frames_1080p_to_the_next_multiple_of_14(lib, ctx, tool):
    import torch
    rng = np.random.default_rng(1899)
    frame = rng.integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)
    d = torch.from_numpy(frame).cuda()
    want = er.model_frames(frame, (1932, 1092), as_float=True)
    got = tool.model_frames(ctx, d, (1932, 1092), as_float=True)
    assert got.shape == (1, 3, 1092, 1932) and mr.same_bits(got.cpu().numpy(), want).size == 0
    got8 = tool.model_frames(ctx, d.flip(-1), (1932, 1092), bgr=True)
    assert np.array_equal(got8.cpu().numpy(), er.model_frames(frame, (1932, 1092)))
    assert np.array_equal(tool.model_frames(ctx, d).cpu().numpy(), frame.transpose(0, 3, 1, 2))


# ---- mdvt_depth_prompt ------------------------------------------------------------------------------------------------------------
def _prompt_body(lib, ctx, codes, out_size, bgr, max_depth, lays):
    L = lib.load()
    N, H, W = codes.shape[:3]
    w, h = out_size
    lin, lout = lays
    lout = fp.Layout(lout.base * 4 % 16, lout.pad * 4 if lout.pad % 4 else lout.pad, lout.gap * 4 if lout.gap % 4 else lout.gap)

    def body(run, **wrong):
        ain = run.inp("codes", codes, lin)
        aout = run.out("prompt", h, 4 * w, N, lout)
        a = dict(ctx=ctx.handle, in_w=W, in_h=H, n=N, codes=_vp(ain), codes_pitch=ain.pitch, codes_stride=ain.stride, order=int(bgr),
                 max_depth=float(max_depth), out_w=w, out_h=h, prompt=_vp(aout), prompt_pitch=aout.pitch, prompt_stride=aout.stride)
        a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})      # (a callable makes its wrong value from the right ones)
        rc = L.mdvt_depth_prompt(a["ctx"], a["in_w"], a["in_h"], a["n"], a["codes"], a["codes_pitch"], a["codes_stride"], a["order"],
                                 a["max_depth"], a["out_w"], a["out_h"], a["prompt"], a["prompt_pitch"], a["prompt_stride"], None)
        if not wrong:
            ctx.check(rc)
        run.vector = fp.all_aligned([aout], 16) and w >= 4
        return rc
    return body


def _depth_codes(rng, N, H, W):
    """Depth frames as a depth video holds them: R = G the high byte, B the low one; codes 0x0000 and 0xFFFF among them."""
    code = rng.integers(0, 1 << 16, (N, H, W))
    code.reshape(-1)[:4] = [0, 0xFFFF, 0x00FF, 0xFF00]
    hi, lo = (code >> 8).astype(np.uint8), (code & 0xFF).astype(np.uint8)
    g = rng.integers(0, 256, (N, H, W), dtype=np.uint8)             # G is ignored: anything
    return np.stack([hi, g, lo], axis=-1)


@pytest.mark.parametrize("size", [((40, 24), (16, 12)), ((8, 6), (8, 6)), ((31, 17), (7, 5))], ids=["40x24->16x12", "8x6->8x6", "31x17->7x5"])
def test_depth_prompt_equals_the_restatement_and_keeps_its_footprint(lib, ctx, size):
    (W, H), (w, h) = size
    rng = np.random.default_rng(1900 + W)
    rgb = _depth_codes(rng, 2, H, W)
    vector = 0
    for max_depth in (100, 20):
        want = er.depth_prompt(rgb, max_depth, (w, h))
        for k, (lays, N, bgr) in enumerate((lays, N, bgr) for lays in (ALIGNED, PADDED16, ODD) for N in (1, 2) for bgr in (0, 1)):
            stored = np.ascontiguousarray(rgb[:N, ..., ::-1] if bgr else rgb[:N])
            body = _prompt_body(lib, ctx, stored, (w, h), bgr, max_depth, lays)
            box = {}

            def accepted(run):
                body(run)
                box["vector"] = run.vector
            tag = f"prompt {N}x{W}x{H}->{w}x{h} bgr={bgr} max_depth={max_depth} {lays}"
            out = fp.twice(PROMPT, accepted, seed=k, what=tag)["prompt"]
            fp.accepted(PROMPT, vector=box["vector"])
            vector += int(box["vector"])
            assert mr.same_bits(np.ascontiguousarray(out).view(F).reshape(N, h, w), want[:N]).size == 0, tag
    assert vector >= 2 or w % 4, "a width that is a multiple of 4 reaches the 16-byte stores"
    fp.finish_entry(PROMPT, need_odd=True, need_padded=True, need_vector=w % 4 == 0)


def test_depth_prompt_1080p_to_256x192(lib, ctx, tool):
    import torch
    rng = np.random.default_rng(1950)
    rgb = _depth_codes(rng, 1, 1080, 1920)
    got = tool.depth_prompt(ctx, torch.from_numpy(rgb).cuda(), 100, (256, 192))
    assert got.shape == (1, 192, 256) and mr.same_bits(got.cpu().numpy(), er.depth_prompt(rgb, 100, (256, 192))).size == 0


# ---- mdvt_focal_from_points ---------------------------------------------------------------------------------------------------------
COUNTS = (0, 5, 129, 8191, 8192, 8193, 9216)


def _pinhole(rng, H, W, fx, fy, noise=0.03):
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    Z = rng.uniform(0.5, 20.0, (H, W))
    X = (u - W / 2.0) * Z / fx * (1.0 + rng.normal(0, noise, (H, W)))
    Y = (v - H / 2.0) * Z / fy * (1.0 + rng.normal(0, noise, (H, W)))
    X[np.abs(X) < 1e-3] = 0.25                                      # the middle column and row would be 0: selected, like the rest
    Y[np.abs(Y) < 1e-3] = -0.25
    return np.stack([X, Y, Z], axis=-1).astype(F)


@pytest.fixture(scope="module")
def counted_frames():
    """Seven 96 x 96 point maps whose selections hold COUNTS[i] values in x and COUNTS[(i + 3) % 7] in y, scattered over the frame, and
    their restated focal lengths: computed once, shared."""
    rng = np.random.default_rng(2000)
    frames = []
    for i in range(len(COUNTS)):
        p = _pinhole(rng, 96, 96, 80.0 + i, 70.0 - i)
        for axis, n in ((0, COUNTS[i]), (1, COUNTS[(i + 3) % len(COUNTS)])):
            off = rng.permutation(96 * 96)[n:]
            p.reshape(-1, 3)[off, axis] = rng.choice(np.array([0.0, -0.0, 1e-7, np.nan], F), off.size)
        frames.append(p)
    frames = np.stack(frames)                                       # [7, 96, 96, 3]
    f, n = er.focal(frames)
    assert n.tolist() == [[COUNTS[i], COUNTS[(i + 3) % 7]] for i in range(7)] and np.isfinite(f).all()
    return frames, f, n


def test_focal_on_both_sides_of_a_chunk_edge_in_both_layouts(lib, ctx, tool, counted_frames):
    import torch
    frames, want_f, want_n = counted_frames
    last = torch.from_numpy(frames).cuda()                          # [7, H, W, 3]
    first = last.permute(0, 3, 1, 2).contiguous()                   # [7, 3, H, W]
    for points in (last, first):
        f, n = tool.focal_from_points(ctx, points, want_counts=True)                   # seven frames in one call
        assert np.array_equal(n.cpu().numpy(), want_n) and mr.same_bits(f.cpu().numpy(), want_f).size == 0
        for i in range(7):                                                             # one frame per call
            f, n = tool.focal_from_points(ctx, points[i:i + 1], want_counts=True)
            assert np.array_equal(n.cpu().numpy(), want_n[i:i + 1]) and mr.same_bits(f.cpu().numpy(), want_f[i:i + 1]).size == 0, i
    # three frames with padded rows, gapped planes and frames, in both layouts
    buf = torch.full((3, 3, 96 + 2, 96 + 5), float("nan"), device="cuda")
    view = buf[:, :, 1:97, 3:99]
    view.copy_(first[3:6])
    buf2 = torch.full((3, 96 + 1, 96 + 3, 3), float("nan"), device="cuda")
    view2 = buf2[:, :96, 2:98]
    view2.copy_(last[3:6])
    for v in (view, view2):
        assert not v.is_contiguous()
        f = tool.focal_from_points(ctx, v)
        assert mr.same_bits(f.cpu().numpy(), want_f[3:6]).size == 0


def test_focal_runs_in_launch_sets_under_a_small_workspace(lib, tool, counted_frames):
    """workspace_mib = 1 affords 14 frames of 96 x 96 (73920 B each): 30 frames are three launch sets, on less than the 2.2 MB that
    one set of 30 would take."""
    import torch
    frames, want_f, want_n = counted_frames
    idx = [k % 7 for k in range(30)]
    ctx = gc.make_context(lib, 16, 16, workspace_mib=1)
    try:
        f, n = tool.focal_from_points(ctx, torch.from_numpy(frames[idx]).cuda(), want_counts=True)
        assert np.array_equal(n.cpu().numpy(), want_n[idx]) and mr.same_bits(f.cpu().numpy(), want_f[idx]).size == 0
        assert ctx.workspace_bytes() < 30 * 73920
    finally:
        ctx.close()


def test_focal_special_values_and_a_7x3_frame(lib, ctx, tool):
    import torch
    g = np.load(os.path.join(REPO, "tests", "golden", "depth_engines.npz"))
    for case in ("special7x3", "empty7x3", "clean40x30"):
        points = g[f"focal_{case}_points"]
        want_f, want_n = er.focal(points)
        f, n = tool.focal_from_points(ctx, torch.from_numpy(points).cuda(), want_counts=True)
        assert np.array_equal(n.cpu().numpy(), want_n) and mr.same_bits(f.cpu().numpy(), want_f).size == 0, case
    # |X| and |Z| at float32(1e-6) and its two neighbours, with both signs; +-0, NaN and +-inf entries -- and a finite mean
    eps = F(1e-6)
    edge = np.array([eps, np.nextafter(eps, F(1)), np.nextafter(eps, F(0))], F)
    rng = np.random.default_rng(2001)
    p = _pinhole(rng, 3, 7, 5.0, 4.0)
    p[0, :3, 0], p[0, 3:6, 0] = edge, -edge
    p[1, :3, 2], p[1, 3:6, 2] = edge, -edge
    p[2, :6, 1] = [0.0, -0.0, np.nan, np.inf, -np.inf, eps]
    want_f, want_n = er.focal(p[None])
    assert want_n[0, 0] == 7 * 3 - 4 - 4 and np.isfinite(want_f[0, 0])   # only the upper neighbours count
    for points in (p[None], np.ascontiguousarray(p.transpose(2, 0, 1))[None]):
        f, n = tool.focal_from_points(ctx, torch.from_numpy(points).cuda(), want_counts=True)
        assert np.array_equal(n.cpu().numpy(), want_n) and mr.same_bits(f.cpu().numpy(), want_f).size == 0


def test_focal_1080p(lib, ctx, tool):
    import torch
    rng = np.random.default_rng(2002)
    p = _pinhole(rng, 1080, 1920, 1400.0, 1390.0)
    drop = rng.random((1080, 1920))
    p[drop < 0.1, 0] = 0.0
    p[drop > 0.95, 2] = np.nan
    want_f, want_n = er.focal(p[None])
    f, n = tool.focal_from_points(ctx, torch.from_numpy(p[None]).cuda(), want_counts=True)
    assert np.array_equal(n.cpu().numpy(), want_n) and want_n[0, 0] != want_n[0, 1] and mr.same_bits(f.cpu().numpy(), want_f).size == 0
    assert abs(float(want_f[0, 0]) - 1400.0) < 5 and abs(float(want_f[0, 1]) - 1390.0) < 5


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(lib, ctx, entry, body, cases):
    L = lib.load()
    for k, (what, wrong, status, text) in enumerate(cases):
        fp.refused(entry, lambda run: body(run, **wrong), status, seed=k)
        got = (L.mdvt_last_error(ctx.handle) or b"").decode()
        assert text in got, f"{entry}, {what}: mdvt_last_error says {got!r}"
    assert fp.tally(entry)["refused"] >= len(cases)


def test_model_frames_refusals_leave_their_text_and_write_nothing(lib, ctx):
    rng = np.random.default_rng(2100)
    N, (W, H), (w, h) = 2, (9, 5), (12, 7)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    none = C.c_void_p(None)
    for fmt in (0, 1):
        e = 4 if fmt else 1
        body = _frames_body(lib, ctx, frames, (w, h), fmt, 0, ALIGNED, plane_gap=False)
        cases = [("NULL frames", dict(frames=none), INVALID, "NULL buffer"), ("NULL out", dict(out=none), INVALID, "NULL buffer"),
                 ("in_w 0", dict(in_w=0), INVALID, "bad size"), ("in_h -1", dict(in_h=-1), INVALID, "bad size"),
                 ("out_w 0", dict(out_w=0), INVALID, "bad size"), ("out_h 0", dict(out_h=0), INVALID, "bad size"),
                 ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"), ("order 2", dict(order=2), INVALID, "order must be"),
                 ("order -1", dict(order=-1), INVALID, "order must be"), ("format 2", dict(format=2), INVALID, "format must be"),
                 ("a short frames pitch", dict(frames_pitch=3 * W - 1), INVALID, "frames_pitch smaller than one row"),
                 ("a short out pitch", dict(out_pitch=e * w - 1), INVALID, "out_pitch smaller than one row"),
                 ("a short plane stride", dict(out_plane_stride=e * w * h - 1), INVALID, "out_plane_stride smaller than one plane"),
                 ("a short frames stride", dict(frames_stride=3 * W * H - 1), INVALID, "stride smaller than one frame"),
                 ("a short out stride", dict(out_stride=3 * e * w * h - 1), INVALID, "stride smaller than one frame"),
                 ("2^31 output pixels", dict(out_w=1 << 16, out_h=1 << 15, out_pitch=e << 16, out_plane_stride=e << 31, out_stride=3 * e << 31),
                  UNSUPPORTED, "frame too large"),
                 ("2^31 input pixels", dict(in_w=1 << 16, in_h=1 << 15, frames_pitch=3 << 16, frames_stride=3 << 31), UNSUPPORTED, "frame too large")]
        if fmt:                                                     # a float32 is stored at its alignment; uint8 planes lie anywhere (the ODD layouts)
            text = "must be multiples of 4"
            cases += [("an out pitch of 4 w + 1", dict(out_pitch=4 * w + 1, out_plane_stride=(4 * w + 4) * h, out_stride=3 * (4 * w + 4) * h), INVALID, text),
                      ("a plane stride off by 2", dict(out_plane_stride=4 * w * h + 2, out_stride=3 * (4 * w * h + 4)), INVALID, text),
                      ("an out stride off by 1", dict(out_stride=3 * 4 * w * h + 1), INVALID, text),
                      ("d_out off by 1", dict(out=_moved("out", 1)), INVALID, text), ("d_out off by 2", dict(out=_moved("out", 2)), INVALID, text)]
        _refused(lib, ctx, FRAMES, body, cases)
        fp.twice(FRAMES, lambda run: body(run), seed=99)            # the context still works after them


def test_depth_prompt_refusals_leave_their_text_and_write_nothing(lib, ctx):
    rng = np.random.default_rng(2101)
    N, (W, H), (w, h) = 2, (9, 5), (6, 4)
    rgb = _depth_codes(rng, N, H, W)
    none = C.c_void_p(None)
    body = _prompt_body(lib, ctx, rgb, (w, h), 0, 100, ALIGNED)
    cases = [("NULL codes", dict(codes=none), INVALID, "NULL buffer"), ("NULL prompt", dict(prompt=none), INVALID, "NULL buffer"),
             ("in_w 0", dict(in_w=0), INVALID, "bad size"), ("in_h 0", dict(in_h=0), INVALID, "bad size"),
             ("out_w -1", dict(out_w=-1), INVALID, "bad size"), ("out_h 0", dict(out_h=0), INVALID, "bad size"),
             ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"), ("order 2", dict(order=2), INVALID, "order must be"),
             ("max_depth 0", dict(max_depth=0.0), INVALID, "max_depth must be > 0"),
             ("max_depth NaN", dict(max_depth=float("nan")), INVALID, "max_depth must be > 0"),
             ("max_depth -1", dict(max_depth=-1.0), INVALID, "max_depth must be > 0"),
             ("a short codes pitch", dict(codes_pitch=3 * W - 1), INVALID, "codes_pitch smaller than one row"),
             ("a short prompt pitch", dict(prompt_pitch=4 * w - 4), INVALID, "prompt_pitch smaller than one row"),
             ("a short codes stride", dict(codes_stride=3 * W * H - 1), INVALID, "stride smaller than one frame"),
             ("a short prompt stride", dict(prompt_stride=4 * w * h - 4), INVALID, "stride smaller than one frame"),
             ("2^31 output pixels", dict(out_w=1 << 16, out_h=1 << 15, prompt_pitch=4 << 16, prompt_stride=4 << 31), UNSUPPORTED, "frame too large")]
    text = "must be multiples of 4"
    cases += [("a prompt pitch of 4 w + 2", dict(prompt_pitch=4 * w + 2, prompt_stride=(4 * w + 4) * h), INVALID, text),
              ("a prompt stride off by 2", dict(prompt_stride=4 * w * h + 2), INVALID, text),
              ("d_prompt off by 1", dict(prompt=_moved("prompt", 1)), INVALID, text)]
    _refused(lib, ctx, PROMPT, body, cases)
    # the exact 2x reduction is OpenCV's area path: refused, untouched
    rgb2 = _depth_codes(rng, N, 2 * h, 2 * w)
    for lays in (ALIGNED, ODD):
        body2 = _prompt_body(lib, ctx, rgb2, (w, h), 0, 100, lays)
        _refused(lib, ctx, PROMPT, body2, [("in = 2 out", dict(in_w=2 * w), UNSUPPORTED, "area path")])     # (the sizes as they are)
    fp.twice(PROMPT, lambda run: body(run), seed=99)


def test_focal_refusals_leave_their_text_and_write_nothing(lib, ctx):
    L = lib.load()
    rng = np.random.default_rng(2102)
    N, W, H = 2, 9, 5
    first = rng.normal(size=(N, 3 * H, W)).astype(F)                # [N, 3, H, W], planes tight
    last = rng.normal(size=(N, H, 3 * W)).astype(F)                 # [N, H, W, 3]
    none = C.c_void_p(None)

    def body_of(layout):
        def body(run, **wrong):
            ain = run.inp("points", last if layout else first, fp.Layout(0, 8, 16))
            af, ac = run.out("focal", 1, 8 * N), run.out("counts", 1, 8 * N)
            a = dict(ctx=ctx.handle, width=W, height=H, n=N, points=_vp(ain), layout=layout, pitch=ain.pitch,
                     plane=H * ain.pitch, stride=ain.stride, focal=_vp(af), counts=_vp(ac))
            a.update({k: v(dict(a)) if callable(v) else v for k, v in wrong.items()})      # (a callable makes its wrong value from the right ones)
            rc = L.mdvt_focal_from_points(a["ctx"], a["width"], a["height"], a["n"], a["points"], a["layout"], a["pitch"], a["plane"],
                                          a["stride"], a["focal"], a["counts"], None)
            if not wrong:
                ctx.check(rc)
            return rc
        return body
    for layout in (0, 1):
        row = (12 if layout else 4) * W
        cases = [("NULL points", dict(points=none), INVALID, "NULL buffer"), ("NULL focal", dict(focal=none), INVALID, "NULL buffer"),
                 ("width 0", dict(width=0), INVALID, "bad point map size"), ("height -1", dict(height=-1), INVALID, "bad point map size"),
                 ("no frame", dict(n=0), INVALID, "n_frames must be >= 1"), ("layout 2", dict(layout=2), INVALID, "layout must be"),
                 ("layout -1", dict(layout=-1), INVALID, "layout must be"),
                 ("a short pitch", dict(pitch=row - 4), INVALID, "points_pitch smaller than one row"),
                 ("a short stride", dict(stride=(1 if layout else 3) * H * (row + 8) - 4), INVALID, "points_stride smaller than one frame"),
                 ("a width above 2^23", dict(width=(1 << 23) + 1, height=1, pitch=1 << 27, plane=1 << 27, stride=1 << 29), UNSUPPORTED, "too large"),
                 ("more than 2^28 points", dict(width=1 << 15, height=(1 << 13) + 1, pitch=1 << 19, plane=1 << 33, stride=1 << 35),
                  UNSUPPORTED, "too large")]
        if layout == 0:
            cases.append(("a short plane stride", dict(plane=H * (row + 8) - 4), INVALID, "points_plane_stride smaller than one plane"))
        text = "must be multiples of 4"
        cases += [("a pitch off by 2", dict(pitch=row + 10, plane=H * (row + 12), stride=3 * H * (row + 12)), INVALID, text),
                  ("a stride off by 2", dict(stride=3 * H * (row + 8) + 18), INVALID, text),
                  ("d_points off by 2", dict(points=_moved("points", 2)), INVALID, text),
                  ("d_focal off by 2", dict(focal=_moved("focal", 2)), INVALID, "4-byte aligned"),
                  ("d_counts off by 1", dict(counts=_moved("counts", 1)), INVALID, "4-byte aligned")]
        if layout == 0:
            cases.append(("a plane stride off by 2", dict(plane=H * (row + 8) + 2, stride=3 * H * (row + 8) + 16), INVALID, text))
        _refused(lib, ctx, FOCAL, body_of(layout), cases)
        out = fp.twice(FOCAL, lambda run: body_of(layout)(run), seed=99)               # the context still works; both outputs are written
        want_f, want_n = er.focal((last.reshape(N, H, W, 3) if layout else first.reshape(N, 3, H, W)))
        assert mr.same_bits(np.ascontiguousarray(out["focal"]).view(F).reshape(N, 2), want_f).size == 0
        assert np.array_equal(np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(N, 2), want_n)
    # d_counts is optional
    import torch
    f = torch.zeros(2, device="cuda")
    p = torch.ones((3, 2, 2), device="cuda")
    ctx.check(L.mdvt_focal_from_points(ctx.handle, 2, 2, 1, p.data_ptr(), 0, 8, 16, 48, f.data_ptr(), None, None))
    torch.cuda.synchronize()
