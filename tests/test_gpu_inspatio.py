"""mdvt_masked_shift_grid (include/mdvt_inspatio.h) through the raw C ABI against tests/inspatio_ref.py, bit for bit: the frames, the
validity planes and the three outputs inside one arena filled with a pseudo-random poison (and, again, with its complement), of which
only the outputs may change."""
import os

import numpy as np
import pytest

import inspatio_ref as ir

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
MARGIN = 256
AUTO, DIRECT, TRANSFORM = 0, 1, 2


@pytest.fixture(scope="module")
def env():
    import torch
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(torch.cuda.current_device(), 16, 16)
    yield torch, _lib.load(), ctx
    ctx.close()


def _up(v, k=256):
    return (v + k - 1) // k * k


class Arena:
    """R, I (rows `pitch` bytes apart), V (rows `vpitch` apart), frames `gap` bytes further apart than they need, each at `base` past a
    256-byte boundary; then d_shift, d_status and d_round_error."""

    def __init__(self, torch, R, I, V, pitch=None, vpitch=None, gap=0, base=0, flip=False, seed=1):
        n, H, W = V.shape
        self.n, self.H, self.W = n, H, W
        self.pitch = 3 * W if pitch is None else pitch
        self.vpitch = W if vpitch is None else vpitch
        self.stride, self.vstride = H * self.pitch + gap, H * self.vpitch + gap
        self.at_R = MARGIN + base
        self.at_I = _up(self.at_R + n * self.stride + MARGIN) + base
        self.at_V = _up(self.at_I + n * self.stride + MARGIN) + base
        self.at_shift = _up(self.at_V + n * self.vstride + MARGIN)
        self.at_status = _up(self.at_shift + 256 * n + MARGIN) + 1
        self.at_err = _up(self.at_status + 16 * n + MARGIN) + 8
        total = self.at_err + 8 + MARGIN
        poison = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
        self.buf = torch.from_numpy(~poison if flip else poison).cuda()
        for at, img, p, st, c in ((self.at_R, R, self.pitch, self.stride, 3), (self.at_I, I, self.pitch, self.stride, 3), (self.at_V, V, self.vpitch, self.vstride, 1)):
            view = torch.as_strided(self.buf, (n, H, W * c), (st, p, 1), at)
            view.copy_(torch.from_numpy(np.ascontiguousarray(img).reshape(n, H, W * c)).cuda())
        self.before = self.buf.cpu().numpy().copy()
        self.ptr = self.buf.data_ptr()

    def args(self, path=AUTO):
        p = self.ptr
        return [self.W, self.H, self.n, p + self.at_R, self.pitch, self.stride, p + self.at_I, self.pitch, self.stride,
                p + self.at_V, self.vpitch, self.vstride, path, p + self.at_shift, p + self.at_status, p + self.at_err]

    def after(self, torch):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def untouched(self, torch):
        return bool((self.after(torch) == self.before).all())

    def outputs(self, torch):
        """(shift, status, round error); asserts that nothing else of the arena changed."""
        got = self.after(torch)
        keep = np.ones(len(got), bool)
        spans = ((self.at_shift, 256 * self.n), (self.at_status, 16 * self.n), (self.at_err, 8))
        for at, size in spans:
            keep[at:at + size] = False
        assert (got[keep] == self.before[keep]).all(), "bytes outside the outputs changed"
        shift = got[spans[0][0]:spans[0][0] + spans[0][1]].copy().view(np.float64).reshape(self.n, 4, 4, 2)
        status = got[spans[1][0]:spans[1][0] + spans[1][1]].copy().reshape(self.n, 4, 4)
        return shift, status, float(got[spans[2][0]:spans[2][0] + 8].copy().view(np.float64)[0])


def _run(env, R, I, V, path=AUTO, **layout):
    torch, L, ctx = env
    a = Arena(torch, R, I, V, **layout)
    rc = L.mdvt_masked_shift_grid(ctx.handle, *a.args(path), None)
    assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
    return a.outputs(torch)


def _same(got, want):
    shift, status, _ = got
    return np.array_equal(status, want[1]) and np.array_equal(shift.view(np.uint64), want[0].view(np.uint64))


def _reference(R, I, V, route=None):
    both = [ir.shift_grid(R[k], I[k], V[k], route) for k in range(len(V))]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def _scene(H, W, seed):
    """Three frames: noise with rectangular holes (about a quarter), blacked in the render; the infilled frames are the render moved
    by (2, -1) and by (-1, 3) with noise under the holes, and unrelated noise."""
    rng = np.random.default_rng(seed)
    V = np.full((3, H, W), 255, np.uint8)
    for k in range(3):
        for _ in range(max(3, H * W // 320)):
            y, x = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 5))
            V[k, y:y + int(rng.integers(2, 9)), x:x + int(rng.integers(2, 11))] = 0
    base = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    R = base.copy()
    R[V == 0] = 0
    I = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    for k, (dy, dx) in enumerate(((2, -1), (-1, 3))):
        moved = np.roll(R[k], (dy, dx), axis=(0, 1))
        hole = np.roll(V[k], (dy, dx), axis=(0, 1)) == 0
        I[k] = np.where(hole[..., None], I[k], moved)
    return R, I, V


SHAPES = [(46, 90), (33, 41)]
_cache = {}


def _scene_and_reference(H, W):
    if (H, W) not in _cache:
        R, I, V = _scene(H, W, H * 1000 + W)
        want = _reference(R, I, V)
        assert _same((*_reference(R, I, V, ir.TRANSFORM), 0.0), want), "the restatement's two routes agree"
        _cache[(H, W)] = (R, I, V, want)
    return _cache[(H, W)]


# (name, pitch(W), validity pitch(W), gap, base)
LAYOUTS = [("contiguous", lambda W: 3 * W, lambda W: W, 0, 0), ("padded", lambda W: 3 * W + 5, lambda W: W + 3, 0, 0),
           ("gapped", lambda W: 3 * W + 16, lambda W: W, 7, 0), ("odd_base", lambda W: 3 * W + 1, lambda W: W + 1, 0, 3)]


@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_shift_grid_equals_the_restatement_in_every_layout(env, H, W, layout):
    torch, L, ctx = env
    _, pitch_of, vpitch_of, gap, base = layout
    R, I, V, want = _scene_and_reference(H, W)
    assert L.mdvt_masked_shift_path(W, H) == DIRECT
    assert want[1][:2, :, 1:3].all() and want[0][0, :, 1:3].reshape(-1, 2).tolist() == [[-2.0, 1.0]] * 8       # the scene means something
    for n in (1, 3):
        for path in (AUTO, DIRECT, TRANSFORM):
            for flip in (False, True):
                got = _run(env, R[:n], I[:n], V[:n], path, pitch=pitch_of(W), vpitch=vpitch_of(W), gap=gap, base=base, flip=flip)
                assert _same(got, (want[0][:n], want[1][:n])), (n, path, flip)
                assert (got[2] == 0.0) if path != TRANSFORM else (0.0 <= got[2] < 1e-6), got[2]


def test_special_contents(env):
    H, W = 46, 90
    R, I, V, _ = _scene_and_reference(H, W)
    R, I, V = R[:1].copy(), I[:1].copy(), V[:1].copy()
    ye, xe = ir.edges(H), ir.edges(W)

    def cell(gy, gx):
        return (0, slice(ye[gy], ye[gy + 1]), slice(xe[gx], xe[gx + 1]))

    V[cell(1, 1)] = 0
    V[0, ye[1], xe[1]:xe[1] + 22] = 255                             # 22 of 12 * 23 = 276 pixels: below 0.2
    V[cell(2, 0)] = 0
    V[0, ye[2]:ye[2] + 2, xe[0]:xe[1]] = 255                        # two of 12 rows: below 0.2
    V[cell(0, 3)] = 0                                               # no valid row
    V[cell(3, 1)] = 255                                             # an all-valid cell
    R[cell(2, 2)] = 0                                               # an all-black render: den = 0, every displacement ties
    R[cell(1, 2)] = (9, 200, 31)                                    # a constant cell in both images
    I[cell(1, 2)] = (9, 200, 31)
    I[cell(3, 3)] = R[cell(3, 3)]                                   # a border cell that matches at 0
    want = _reference(R, I, V)
    assert want[1][0].tolist() == [[1, 1, 1, 0], [1, 0, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]]
    assert want[0][0, 2, 2].tolist() == [0.0, 0.0] and want[0][0, 1, 2].tolist() == [0.0, 0.0] and want[0][0, 3, 3].tolist() == [0.0, 0.0]
    for path in (DIRECT, TRANSFORM):
        for flip in (False, True):
            assert _same(_run(env, R, I, V, path, flip=flip), want), (path, flip)
    # an all-valid frame
    V[:] = 255
    want = _reference(R, I, V)
    assert want[1].all()
    for path in (DIRECT, TRANSFORM):
        assert _same(_run(env, R, I, V, path), want), path


def test_tied_maxima_take_the_mean(env):
    """Images of period 4 along x and along y in fully valid cells: the maxima tie at every multiple of 4 whose overlap keeps 0.3 of
    the cell, on both sides of 0, and the shift is the mean of all of them; the infilled frame moved by one column moves the mean."""
    H, W = 48, 96
    yy, xx = np.mgrid[0:H, 0:W]
    g = (np.array([10, 200, 90, 30])[xx % 4] + np.array([0, 17, 3, 40])[yy % 4]).astype(np.uint8)
    R = np.repeat(g[None, :, :, None], 3, axis=3)
    I = np.roll(R, 1, axis=2)
    V = np.full((1, H, W), 255, np.uint8)
    want = _reference(R, I, V)
    # 24 maxima of c = 1 in a 12 x 24 cell: dy in (-8 .. 8), dx in (-15 .. 13) in steps of 4 where the overlap allows; their mean is no integer
    assert want[1].all() and want[0][0, :, 1:3, 0].tolist() == [[0.0, 0.0]] * 4 and set(want[0][0, :, 1:3, 1].reshape(-1).tolist()) == {-1.0 / 3.0}
    for path in (DIRECT, TRANSFORM):
        assert _same(_run(env, R, I, V, path), want), path


@pytest.fixture(scope="module")
def eye_1080():
    """One 1080 x 960 eye of noise with holes, the infilled frame its render moved by (-4, 6); and its reference, made once."""
    rng = np.random.default_rng(1080960)
    H, W = 1080, 960
    V = np.full((1, H, W), 255, np.uint8)
    for _ in range(300):
        y, x = int(rng.integers(0, H - 60)), int(rng.integers(0, W - 40))
        V[0, y:y + int(rng.integers(8, 60)), x:x + int(rng.integers(8, 40))] = 0
    R = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    R[V == 0] = 0
    I = np.roll(R, (-4, 6), axis=(1, 2))
    return R, I, V, _reference(R, I, V)


def test_a_1080p_eye_of_noise_on_the_transform_path(env, eye_1080):
    torch, L, ctx = env
    R, I, V, want = eye_1080
    assert L.mdvt_masked_shift_path(960, 1080) == TRANSFORM == ir.path_of(960, 1080)
    assert want[1].all() and want[0][0, :, 1:3].reshape(-1, 2).tolist() == [[4.0, -6.0]] * 8
    for path in (AUTO, TRANSFORM):
        got = _run(env, R, I, V, path, pitch=3 * 960 + 32)
        print(f"1080 x 960 noise, path {path}: largest distance from an integer {got[2]:.3g}")
        assert _same(got, want) and 0.0 < got[2] < 0.25


def test_a_1080p_eye_all_255_and_fully_valid(env):
    H, W = 1080, 960
    R = np.full((1, H, W, 3), 255, np.uint8)
    V = np.full((1, H, W), 255, np.uint8)
    got = _run(env, R, R, V, TRANSFORM)
    print(f"1080 x 960 all 255: largest distance from an integer {got[2]:.3g}")
    # every sum is a multiple of its overlap: num = 0 and den = 0 at every displacement, every displacement ties, the mean is 0
    assert got[1].all() and not got[0].any() and not np.signbit(got[0]).any() and 0.0 < got[2] < 0.25


def test_the_largest_supported_cell_keeps_the_sums_exact(env):
    """A 4096 x 4096 eye, all 255 and fully valid: cells of 1024 x 1024, the sums up to 255^2 * 2^20, transforms of 2048 x 2048.  The
    frames are made on the device; the expected result is the definition's, as for the 1080p eye."""
    torch, L, ctx = env
    H = W = 4096
    R = torch.full((H, W, 3), 255, dtype=torch.uint8, device="cuda")
    V = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
    out = torch.full((32 + 2 + 1 + 1,), -1.0, dtype=torch.float64, device="cuda")       # shift, status, the rounding distance, a guard
    p = out.data_ptr()
    assert L.mdvt_masked_shift_path(W, H) == TRANSFORM
    rc = L.mdvt_masked_shift_grid(ctx.handle, W, H, 1, R.data_ptr(), 3 * W, 0, R.data_ptr(), 3 * W, 0, V.data_ptr(), W, 0, AUTO, p, p + 256, p + 272, None)
    assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print(f"4096 x 4096 all 255: largest distance from an integer {got[34]:.3g}")
    assert not got[:32].any() and got[32:34].view(np.uint8).tolist() == [1] * 16 and got[35] == -1.0
    assert 0.0 < got[34] < 0.25


def test_the_largest_cell_finds_a_known_shift_of_noise(env):
    """A 4096 x 4096 eye of noise, about a fifth of it holes, the infilled frame the render moved cyclically by (5, -7): the peak of
    every interior cell of 1024 x 1024 is at d = (5, -7) alone, so the sums of the largest supported cell decide the result: (-5, 7)."""
    torch, L, ctx = env
    H = W = 4096
    g = torch.Generator(device="cuda").manual_seed(4096)
    V = (torch.rand((H, W), generator=g, device="cuda") < 0.8).to(torch.uint8) * 255
    R = torch.randint(0, 256, (H, W, 3), generator=g, device="cuda", dtype=torch.uint8) * (V != 0)[..., None]
    I = torch.roll(R, (5, -7), dims=(0, 1))
    out = torch.full((32 + 2 + 1 + 1,), -1.0, dtype=torch.float64, device="cuda")
    p = out.data_ptr()
    rc = L.mdvt_masked_shift_grid(ctx.handle, W, H, 1, R.data_ptr(), 3 * W, 0, I.data_ptr(), 3 * W, 0, V.data_ptr(), W, 0, AUTO, p, p + 256, p + 272, None)
    assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print(f"4096 x 4096 noise: largest distance from an integer {got[34]:.3g}")
    assert got[:32].reshape(4, 4, 2)[:, 1:3].reshape(-1, 2).tolist() == [[-5.0, 7.0]] * 8
    assert got[32:34].view(np.uint8).tolist() == [1] * 16 and got[35] == -1.0 and 0.0 < got[34] < 0.25


REFUSALS = [
    ("null render", dict(null=3), INVALID, "NULL buffer"),
    ("null infilled", dict(null=6), INVALID, "NULL buffer"),
    ("null valid", dict(null=9), INVALID, "NULL buffer"),
    ("null shift", dict(null=13), INVALID, "NULL buffer"),
    ("null status", dict(null=14), INVALID, "NULL buffer"),
    ("misaligned shift", dict(off=(13, 4)), INVALID, "must be 8-byte aligned"),
    ("misaligned round error", dict(off=(15, 2)), INVALID, "must be 8-byte aligned"),
    ("width 0", dict(set={0: 0}), INVALID, "bad size 0 x 16"),
    ("n_frames 0", dict(set={2: 0}), INVALID, "n_frames must be >= 1"),
    ("render pitch", dict(set={4: 3 * 16 - 1}), INVALID, "render_pitch smaller than one row"),
    ("infilled pitch", dict(set={7: 3 * 16 - 1}), INVALID, "infilled_pitch smaller than one row"),
    ("valid pitch", dict(set={10: 15}), INVALID, "valid_pitch smaller than one row"),
    ("render stride", dict(set={5: 16 * 48 - 1}), INVALID, "stride smaller than one frame"),
    ("valid stride", dict(set={11: 16 * 16 - 1}), INVALID, "stride smaller than one frame"),
    ("path 3", dict(set={12: 3}), INVALID, "path must be 0 (auto), 1 (direct) or 2 (transform), got 3"),
    ("7 wide", dict(set={0: 7}), UNSUPPORTED, "an eye below 8 x 8 (7 x 16)"),
    ("7 high", dict(set={1: 7}), UNSUPPORTED, "an eye below 8 x 8 (16 x 7)"),
    ("4097 wide", dict(set={0: 4097, 4: 3 * 4097, 7: 3 * 4097, 10: 4097, 5: 16 * 3 * 4097, 8: 16 * 3 * 4097, 11: 16 * 4097}), UNSUPPORTED, "a cell side above 1024"),
    ("4097 high", dict(set={1: 4097, 5: 4097 * 48, 8: 4097 * 48, 11: 4097 * 16}), UNSUPPORTED, "a cell side above 1024"),
    ("direct beyond the LDS", dict(set={0: 516, 1: 512, 12: 1, 4: 3 * 516, 7: 3 * 516, 10: 516, 5: 512 * 3 * 516, 8: 512 * 3 * 516, 11: 512 * 516}),
     UNSUPPORTED, "the direct path holds a cell of at most 16384 pixels"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_arena_untouched(env, case):
    torch, L, ctx = env
    _, ch, code, text = case
    rng = np.random.default_rng(3)
    R, I = rng.integers(0, 256, (2, 2, 16, 16, 3), dtype=np.uint8)
    V = np.full((2, 16, 16), 255, np.uint8)
    a = Arena(torch, R, I, V)
    args = a.args()
    if "null" in ch:
        args[ch["null"]] = None
    if "off" in ch:
        args[ch["off"][0]] += ch["off"][1]
    for at, v in ch.get("set", {}).items():
        args[at] = v
    rc = L.mdvt_masked_shift_grid(ctx.handle, *args, None)
    got = (L.mdvt_last_error(ctx.handle) or b"").decode()
    assert rc == code and text in got, (rc, got)
    assert a.untouched(torch)
    # the context is usable afterwards
    rc = L.mdvt_masked_shift_grid(ctx.handle, *a.args(), None)
    assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
    assert _same(a.outputs(torch), _reference(R, I, V))


def test_the_smallest_eye_and_the_last_sizes_accepted(env):
    """8 x 8 runs (cells of 2 x 2) on both paths; 4096 is accepted by the argument check's own function (the largest cell runs in
    test_the_largest_supported_cell_keeps_the_sums_exact); the direct path's largest cell, 128 x 128, runs."""
    torch, L, ctx = env
    rng = np.random.default_rng(8)
    R, I = rng.integers(0, 256, (2, 1, 8, 8, 3), dtype=np.uint8)
    V = (rng.random((1, 8, 8)) < 0.8).astype(np.uint8)
    want = _reference(R, I, V)
    for path in (AUTO, DIRECT, TRANSFORM):
        assert _same(_run(env, R, I, V, path), want), path
    assert L.mdvt_masked_shift_path(4096, 4096) == TRANSFORM and L.mdvt_masked_shift_path(4097, 4096) == 0
    H = W = 512
    R = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    V = (rng.random((1, H, W)) < 0.6).astype(np.uint8)
    R[V == 0] = 0
    I = np.roll(R, (1, -2), axis=(1, 2))
    got = _run(env, R, I, V, TRANSFORM)
    assert got[1].all() and got[0][0, :, 1:3].reshape(-1, 2).tolist() == [[-1.0, 2.0]] * 8
    assert _same(_run(env, R, I, V, DIRECT), got[:2]), "a cell of 16384 pixels: the two paths agree"


def test_the_wrapper_checks_its_tensors_and_enqueues(env):
    torch, L, ctx = env
    from metric_depth_video_toolbox_amd import inspatio_device as idev
    H, W = 33, 41
    R, I, V, want = _scene_and_reference(H, W)
    wide = torch.zeros((3, H, W + 7, 3), dtype=torch.uint8, device="cuda")
    r, i, v = wide[:, :, 2:2 + W], torch.from_numpy(I).cuda(), torch.from_numpy(V).cuda()
    r.copy_(torch.from_numpy(R).cuda())
    for path in (AUTO, TRANSFORM):
        shift, status, err = idev.masked_shift_grid(ctx, r, i, v, path=path)
        assert shift.dtype == torch.float64 and tuple(shift.shape) == (3, 4, 4, 2) and status.dtype == torch.uint8
        assert _same((shift.cpu().numpy(), status.cpu().numpy(), 0.0), want) and 0.0 <= float(err.cpu()[0]) < 0.25
    with pytest.raises(ValueError, match="render must be on a GPU"):
        idev.masked_shift_grid(ctx, r.cpu(), i, v)
    with pytest.raises(ValueError, match="valid must be"):
        idev.masked_shift_grid(ctx, r, i, v[:, :-1])
    with pytest.raises(TypeError, match="infilled must be"):
        idev.masked_shift_grid(ctx, r, i.float(), v)
    with pytest.raises(ValueError, match="path must be"):
        idev.masked_shift_grid(ctx, r, i, v, path=3)
