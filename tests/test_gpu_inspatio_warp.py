"""mdvt_flow_warp (include/mdvt_inspatio.h) through the raw C ABI against tests/inspatio_ref.py's warp, bit for bit: the grids, the
flags, the infilled frames and the output inside one arena of pseudo-random poison (and, again, of its complement), of which only the
first 3 * width bytes of the output's rows may change."""
import os

import numpy as np
import pytest

import inspatio_ref as ir

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
MARGIN = 256
F = np.float32


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
    def __init__(self, torch, grids, has, frames, pitch=None, out_pitch=None, gap=0, base=0, flip=False, seed=2):
        n, H, W, _ = frames.shape
        self.n, self.H, self.W = n, H, W
        self.pitch = 3 * W if pitch is None else pitch
        self.out_pitch = 3 * W if out_pitch is None else out_pitch
        self.stride, self.out_stride = H * self.pitch + gap, H * self.out_pitch + gap
        self.at_grids = MARGIN
        self.at_has = _up(self.at_grids + 128 * n + MARGIN) + 1
        self.at_src = _up(self.at_has + n + MARGIN) + base
        self.at_out = _up(self.at_src + n * self.stride + MARGIN) + base
        total = self.at_out + n * self.out_stride + MARGIN
        poison = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
        host = ~poison if flip else poison
        host[self.at_grids:self.at_grids + 128 * n] = np.ascontiguousarray(grids, F).view(np.uint8).reshape(-1)
        host[self.at_has:self.at_has + n] = np.asarray(has, np.uint8)
        self.buf = torch.from_numpy(host).cuda()
        torch.as_strided(self.buf, (n, H, 3 * W), (self.stride, self.pitch, 1), self.at_src).copy_(torch.from_numpy(np.ascontiguousarray(frames).reshape(n, H, 3 * W)).cuda())
        self.before = self.buf.cpu().numpy().copy()
        self.ptr = self.buf.data_ptr()

    def args(self):
        p = self.ptr
        return [self.W, self.H, self.n, p + self.at_grids, p + self.at_has, p + self.at_src, self.pitch, self.stride, p + self.at_out, self.out_pitch, self.out_stride]

    def after(self, torch):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def untouched(self, torch):
        return bool((self.after(torch) == self.before).all())

    def output(self, torch):
        got = self.after(torch)
        keep = np.ones(len(got), bool)
        out = np.zeros((self.n, self.H, 3 * self.W), np.uint8)
        for k in range(self.n):
            for y in range(self.H):
                at = self.at_out + k * self.out_stride + y * self.out_pitch
                keep[at:at + 3 * self.W] = False
                out[k, y] = got[at:at + 3 * self.W]
        assert (got[keep] == self.before[keep]).all(), "bytes outside the output rows changed"
        return out.reshape(self.n, self.H, self.W, 3)


def _run(env, grids, has, frames, **layout):
    torch, L, ctx = env
    a = Arena(torch, grids, has, frames, **layout)
    rc = L.mdvt_flow_warp(ctx.handle, *a.args(), None)
    assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
    return a.output(torch)


def _want(grids, has, frames):
    return np.stack([ir.warp(frames[k], grids[k]) if has[k] else frames[k] for k in range(len(frames))])


def _noise(rng, n, H, W):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def test_zero_flow_gives_the_input_bytes(env):
    rng = np.random.default_rng(1)
    frames = _noise(rng, 2, 33, 41)
    grids = np.zeros((2, 4, 4, 2), F)
    for flip in (False, True):
        got = _run(env, grids, [1, 1], frames, pitch=3 * 41 + 5, out_pitch=3 * 41 + 2, gap=7, base=3, flip=flip)
        assert np.array_equal(got, frames) and np.array_equal(_want(grids, [1, 1], frames), frames)


def test_a_uniform_integer_flow_gives_the_clamped_shift(env):
    rng = np.random.default_rng(2)
    H, W = 46, 90
    frames = _noise(rng, 1, H, W)
    for dx, dy in ((3, 0), (0, -2), (-5, 4), (100, -100)):
        grids = np.zeros((1, 4, 4, 2), F)
        grids[..., 0], grids[..., 1] = dx, dy
        ys = np.clip(np.arange(H) - dy, 0, H - 1)
        xs = np.clip(np.arange(W) - dx, 0, W - 1)
        want = frames[:, ys][:, :, xs]
        got = _run(env, grids, [1], frames)
        assert np.array_equal(got, want) and np.array_equal(_want(grids, [1], frames), want), (dx, dy)


@pytest.mark.parametrize("H,W", [(33, 41), (46, 90)], ids=["33x41", "46x90"])
def test_fractional_grids_and_a_frame_without_a_grid(env, H, W):
    rng = np.random.default_rng(H * W)
    frames = _noise(rng, 3, H, W)
    grids = (rng.random((3, 4, 4, 2)) * 12 - 6).astype(F)
    grids[2, 1, 2] = (19.75, -20.0)
    has = [1, 0, 1]
    want = _want(grids, has, frames)
    assert np.array_equal(want[1], frames[1]) and (want[0] != frames[0]).mean() > 0.5
    for layout in (dict(), dict(pitch=3 * W + 5, out_pitch=3 * W + 16, gap=0), dict(pitch=3 * W + 1, out_pitch=3 * W + 1, gap=9, base=1)):
        for flip in (False, True):
            assert np.array_equal(_run(env, grids, has, frames, flip=flip, **layout), want), (layout, flip)
    assert np.array_equal(_run(env, grids[:1], has[:1], frames[:1]), want[:1])          # one frame: its stride is not used


def test_the_u8_rounding_at_taps_0_and_255(env):
    """Frames of 0 and 255 only under fractional flows: every weight pattern of the four taps meets both values; the result is
    (255 * (sum of the weights of the white taps) + 2^14) >> 15 and never leaves [0, 255]."""
    rng = np.random.default_rng(255)
    H, W = 33, 41
    frames = (rng.integers(0, 2, (2, H, W, 1), dtype=np.uint8) * 255).repeat(3, axis=3)
    frames[1] = 255
    grids = (rng.integers(-64, 65, (2, 4, 4, 2)) / 32.0).astype(F)
    got = _run(env, grids, [1, 1], frames)
    assert np.array_equal(got, _want(grids, [1, 1], frames))
    assert (got[1] == 255).all() and len(np.unique(got[0])) > 20


REFUSALS = [
    ("null grids", dict(null=3), INVALID, "NULL buffer"), ("null flags", dict(null=4), INVALID, "NULL buffer"),
    ("null infilled", dict(null=5), INVALID, "NULL buffer"), ("null out", dict(null=8), INVALID, "NULL buffer"),
    ("misaligned grids", dict(off=(3, 2)), INVALID, "d_grids must be 4-byte aligned"),
    ("height 0", dict(set={1: 0}), INVALID, "bad size 16 x 0"), ("n_frames 0", dict(set={2: 0}), INVALID, "n_frames must be >= 1"),
    ("infilled pitch", dict(set={6: 47}), INVALID, "infilled_pitch smaller than one row"),
    ("out pitch", dict(set={9: 47}), INVALID, "out_pitch smaller than one row"),
    ("infilled stride", dict(set={7: 12 * 48 - 1}), INVALID, "stride smaller than one frame"),
    ("out stride", dict(set={10: 12 * 48 - 1}), INVALID, "stride smaller than one frame"),
    ("2^31 pixels", dict(set={0: 1 << 16, 1: 1 << 15, 6: 3 << 16, 9: 3 << 16, 7: 3 << 31, 10: 3 << 31}), UNSUPPORTED, "frame too large"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_arena_untouched(env, case):
    torch, L, ctx = env
    _, ch, code, text = case
    rng = np.random.default_rng(4)
    frames = _noise(rng, 2, 12, 16)
    grids = (rng.random((2, 4, 4, 2)) * 4 - 2).astype(F)
    a = Arena(torch, grids, [1, 1], frames)
    args = a.args()
    if "null" in ch:
        args[ch["null"]] = None
    if "off" in ch:
        args[ch["off"][0]] += ch["off"][1]
    for at, v in ch.get("set", {}).items():
        args[at] = v
    rc = L.mdvt_flow_warp(ctx.handle, *args, None)
    got = (L.mdvt_last_error(ctx.handle) or b"").decode()
    assert rc == code and text in got, (rc, got)
    assert a.untouched(torch)
    assert L.mdvt_flow_warp(ctx.handle, *a.args(), None) == 0
    assert np.array_equal(a.output(torch), _want(grids, [1, 1], frames))


def test_the_wrapper_and_the_whole_alignment_of_a_moved_frame(env):
    """Shifts on the device, the clean-up on the host, the warp on the device: a frame that shows the render from three rows further
    down comes back as the render outside a margin of three rows."""
    torch, L, ctx = env
    from metric_depth_video_toolbox_amd import inspatio_device as idev, inspatio_world
    import test_inspatio_cpu as cpu
    R, I, V = cpu._shifted_scene(7)
    r, i, v = (torch.from_numpy(x[None]).cuda() for x in (R, I, V))
    shift, status, _ = idev.masked_shift_grid(ctx, r, i, v)
    grids, has = inspatio_world.flow_grids(shift.cpu().numpy(), status.cpu().numpy(), [int((V == 0).sum())])
    assert has.tolist() == [1] and np.array_equal(grids[0], np.broadcast_to(np.array([0, 3], F), (4, 4, 2)))
    out = idev.flow_warp(ctx, torch.from_numpy(grids).cuda(), torch.from_numpy(has).cuda(), i)
    assert np.array_equal(out.cpu().numpy()[0, 3:], R[3:])
    with pytest.raises(ValueError, match="grids must be"):
        idev.flow_warp(ctx, torch.zeros((2, 4, 4, 2), device="cuda"), torch.from_numpy(has).cuda(), i)
    with pytest.raises(TypeError, match="has_grid must be"):
        idev.flow_warp(ctx, torch.from_numpy(grids).cuda(), torch.ones(1, device="cuda"), i)
