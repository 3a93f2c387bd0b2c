"""mdvt_inspatio_composite_eye (include/mdvt_inspatio.h) through the raw C ABI against tests/inspatio_ref.py's composite_eye (the C
oracle's mark_lower_side, SciPy's dilation, the 5 x 5 Gaussian restated), bit for bit, in arenas of pseudo-random poison and of its
complement: only the eye's half of the rows of the two outputs may change."""
import numpy as np
import pytest

import inspatio_ref as ir
from test_gpu_inspatio_prepare import Arena, _clip

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def env():
    import torch
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(torch.cuda.current_device(), 16, 16)
    yield torch, _lib.load(), ctx
    ctx.close()


def _arena(env, aligned, color, mask, **layout):
    torch = env[0]
    n, H, W, _ = aligned.shape
    return Arena(torch, dict(aligned=(n, H, 3 * W, aligned), color=(n, H, 6 * W, color), mask=(n, H, 6 * W, mask),
                             pasted=(n, H, 6 * W, None), blended=(n, H, 6 * W, None)), **layout)


def _args(a, W, H, n, eye, blend=True):
    return [W, H, n, eye, *a.triple("aligned"), *a.triple("color"), *a.triple("mask"), *a.triple("pasted"),
            *(a.triple("blended") if blend else [None, 0, 0])]


def _halves(a, name, eye, W):
    """(the eye's half of the output as written, True if the other half still holds the arena's poison)"""
    n, rows, width, pitch, stride, off = a.at[name]
    got = a.read(holes=False)[name]
    before = np.stack([[a.before[off + k * stride + y * pitch: off + k * stride + y * pitch + width] for y in range(rows)] for k in range(n)])
    mine = slice(eye * 3 * W, (eye + 1) * 3 * W)
    other = slice((1 - eye) * 3 * W, (2 - eye) * 3 * W)
    return got[:, :, mine].reshape(n, rows, W, 3), bool((got[:, :, other] == before[:, :, other]).all())


SHAPES = [(33, 41), (46, 90)]


@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_composite_equals_the_restatement_with_and_without_blending(env, orc, H, W):
    torch, L, ctx = env
    rng = np.random.default_rng(H * W + 1)
    color, mask = _clip(rng, 3, H, W)                               # holes on the border of frame 0, one-channel mask pixels
    aligned = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    for eye in (0, 1):
        want = [ir.composite_eye(aligned[k], color[k], mask[k], eye, orc) for k in range(3)]
        assert any((w[0] != w[1]).any() for w in want), "the blend changes something"
        for n, layout in ((3, dict()), (3, dict(pad=5, gap=7, base=3)), (1, dict(pad=16))):
            for blend in (True, False):
                for flip in (False, True):
                    a = _arena(env, aligned[:n], color[:n], mask[:n], flip=flip, **layout)
                    rc = L.mdvt_inspatio_composite_eye(ctx.handle, *_args(a, W, H, n, eye, blend), None)
                    assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
                    pasted, rest = _halves(a, "pasted", eye, W)
                    assert rest and np.array_equal(pasted, np.stack([w[0] for w in want[:n]])), (eye, n, blend, flip)
                    blended, rest = _halves(a, "blended", eye, W)
                    if blend:
                        assert rest and np.array_equal(blended, np.stack([w[1] for w in want[:n]])), (eye, n, flip)
                    else:
                        n_, rows, width, pitch, stride, off = a.at["blended"]
                        assert rest and (a.read(holes=False)["blended"].reshape(-1) ==
                                         np.concatenate([a.before[off + k * stride + y * pitch: off + k * stride + y * pitch + width]
                                                         for k in range(n_) for y in range(rows)])).all(), "no blending: nothing of it is written"


def test_a_frame_without_holes_and_extreme_values(env, orc):
    """No hole: pasted and blended are the render.  Aligned 255 over a render of 0 and the reverse: the blend stays inside [0, 255]
    and reaches both ends."""
    torch, L, ctx = env
    H, W = 20, 24
    rng = np.random.default_rng(3)
    color, mask = _clip(rng, 2, H, W)
    mask[0] = 0
    color[1, :, :W] = 0
    aligned = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    aligned[1] = 255
    a = _arena(env, aligned, color, mask)
    assert L.mdvt_inspatio_composite_eye(ctx.handle, *_args(a, W, H, 2, 0), None) == 0
    pasted, _ = _halves(a, "pasted", 0, W)
    blended, _ = _halves(a, "blended", 0, W)
    assert np.array_equal(pasted[0], color[0, :, :W]) and np.array_equal(blended[0], color[0, :, :W])
    want = ir.composite_eye(aligned[1], color[1], mask[1], 0, orc)
    assert np.array_equal(pasted[1], want[0]) and np.array_equal(blended[1], want[1])
    assert blended[1].min() == 0 and blended[1].max() == 255 and len(np.unique(blended[1])) > 4


REFUSALS = [
    ("null aligned", {4: None}, INVALID, "NULL buffer"), ("null color", {7: None}, INVALID, "NULL buffer"), ("null mask", {10: None}, INVALID, "NULL buffer"),
    ("null pasted", {13: None}, INVALID, "NULL buffer"), ("eye -1", {3: -1}, INVALID, "eye must be 0 (left half) or 1 (right half), got -1"),
    ("height 0", {1: 0}, INVALID, "bad size 24 x 0"), ("n_frames 0", {2: 0}, INVALID, "n_frames must be >= 1"),
    ("aligned pitch", {5: 71}, INVALID, "aligned_pitch smaller than one row"), ("mask pitch", {11: 143}, INVALID, "pitch smaller than one side-by-side row"),
    ("blended pitch", {17: 143}, INVALID, "pitch smaller than one side-by-side row"), ("pasted stride", {15: 20 * 144 - 1}, INVALID, "stride smaller than one frame"),
    ("7 wide", {0: 7}, UNSUPPORTED, "an eye below 8 x 8 (7 x 20)"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_arena_untouched(env, orc, case):
    torch, L, ctx = env
    _, change, code, text = case
    H, W = 20, 24
    rng = np.random.default_rng(11)
    color, mask = _clip(rng, 2, H, W)
    aligned = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    a = _arena(env, aligned, color, mask)
    args = _args(a, W, H, 2, 1)
    bad = list(args)
    for at, v in change.items():
        bad[at] = v
    rc = L.mdvt_inspatio_composite_eye(ctx.handle, *bad, None)
    got = (L.mdvt_last_error(ctx.handle) or b"").decode()
    assert rc == code and text in got, (rc, got)
    assert a.untouched()
    assert L.mdvt_inspatio_composite_eye(ctx.handle, *args, None) == 0
    blended, rest = _halves(a, "blended", 1, W)
    assert rest and np.array_equal(blended, np.stack([ir.composite_eye(aligned[k], color[k], mask[k], 1, orc)[1] for k in range(2)]))
