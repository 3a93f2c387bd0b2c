"""mdvt_scene_frame_sums (include/mdvt_scene.h) through the raw C ABI against tests/scene_ref.py: the three integer sums of every
frame pair bit for bit, with frames, previous frame and d_sums inside one poisoned arena of which only the 3 * pairs words change."""
import ctypes as C

import numpy as np
import pytest

import scene_ref as sr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
POISON = 0xA5
MARGIN = 256


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
    """frames (at `base` past a 256-byte boundary, rows `pitch` and frames `stride` bytes apart), the previous frame and the sums in
    one poisoned buffer."""

    def __init__(self, torch, frames, prev, pitch, stride, base, prev_pitch, prev_base, poison=POISON):
        n, H, W, _ = frames.shape
        self.n, self.H, self.W, self.pitch, self.stride, self.prev_pitch = n, H, W, pitch, stride, prev_pitch
        self.pairs = n - 1 + (prev is not None)
        self.at_frames = MARGIN + base
        self.at_prev = _up(self.at_frames + max(n - 1, 0) * stride + H * max(pitch, 3 * W) + MARGIN) + prev_base
        self.at_sums = _up(self.at_prev + (H * max(prev_pitch, 3 * W) if prev is not None else 0) + MARGIN)
        total = self.at_sums + 24 * max(self.pairs, 1) + MARGIN
        self.buf = torch.full((total,), poison, dtype=torch.uint8, device="cuda")
        if pitch >= 3 * W and (n == 1 or stride >= H * pitch):
            torch.as_strided(self.buf, (n, H, W, 3), (stride, pitch, 3, 1), self.at_frames).copy_(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
        if prev is not None and prev_pitch >= 3 * W:
            torch.as_strided(self.buf, (H, W, 3), (prev_pitch, 3, 1), self.at_prev).copy_(torch.from_numpy(np.ascontiguousarray(prev)).cuda())
        self.has_prev = prev is not None
        self.before = self.buf.cpu().numpy().copy()
        self.ptr = self.buf.data_ptr()

    def args(self, order=0, factor=1):
        return [self.W, self.H, self.n, self.ptr + self.at_frames, self.pitch, self.stride, order,
                (self.ptr + self.at_prev) if self.has_prev else None, self.prev_pitch if self.has_prev else 0, factor, self.ptr + self.at_sums]

    def vector_path(self, L, factor=1):
        return L.mdvt_scene_vector_path(self.n, self.ptr + self.at_frames, self.pitch, self.stride,
                                        (self.ptr + self.at_prev) if self.has_prev else None, self.prev_pitch if self.has_prev else 0, factor)

    def after(self, torch):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def sums(self, torch):
        """The written words; asserts that nothing else of the arena changed."""
        got = self.after(torch)
        lo, hi = self.at_sums, self.at_sums + 24 * self.pairs
        assert (got[:lo] == self.before[:lo]).all() and (got[hi:] == self.before[hi:]).all(), "bytes outside d_sums changed"
        return got[lo:hi].view(np.uint64).reshape(self.pairs, 3).tolist()

    def untouched(self, torch):
        return bool((self.after(torch) == self.before).all())


def _call(env, arena, order=0, factor=1):
    torch, L, ctx = env
    rc = L.mdvt_scene_frame_sums(ctx.handle, *arena.args(order, factor), None)
    text = (L.mdvt_last_error(ctx.handle) or b"").decode()
    return rc, text


def _run(env, frames, prev=None, *, pitch=None, stride=None, base=0, prev_pitch=None, prev_base=0, order=0, factor=1, vec=None, poison=POISON):
    torch, L, ctx = env
    n, H, W, _ = frames.shape
    pitch = 3 * W if pitch is None else pitch
    stride = H * pitch if stride is None else stride
    prev_pitch = pitch if prev_pitch is None else prev_pitch
    a = Arena(torch, frames, prev, pitch, stride, base, prev_pitch, prev_base, poison)
    if vec is not None:
        assert a.vector_path(L, factor) == int(vec), "the layout does not reach the path the test is about"
    rc, text = _call(env, a, order, factor)
    assert rc == 0, text
    return a.sums(torch)


def _noise(rng, n, H, W):
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _up16(v):
    return (v + 15) // 16 * 16


# (name, pitch(W), extra stride, base, previous frame's pitch(W), its base, reaches the 16-byte path)
LAYOUTS = [
    ("contiguous", lambda W: 3 * W, 0, 0, lambda W: 3 * W, 0, None),          # 16-byte path exactly where 3 W is a multiple of 16
    ("pitch16", lambda W: _up16(3 * W + 1), 0, 0, lambda W: _up16(3 * W) + 32, 0, True),
    ("pitch16_gap16", lambda W: _up16(3 * W + 1), 48, 0, lambda W: _up16(3 * W + 1), 16, True),
    ("padded", lambda W: 3 * W + 5, 0, 0, lambda W: 3 * W + 2, 0, False),
    ("gapped", lambda W: _up16(3 * W + 1), 7, 0, lambda W: _up16(3 * W + 1), 0, False),
    ("odd_base", lambda W: _up16(3 * W + 1), 0, 1, lambda W: _up16(3 * W + 1), 0, False),
    ("odd_prev", lambda W: _up16(3 * W + 1), 0, 0, lambda W: _up16(3 * W + 1), 3, None),           # byte path where there is a previous frame
]
SHAPES = [(33, 5), (36, 6), (64, 16)]


@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_sums_equal_the_restatement_in_every_layout(env, W, H, layout):
    name, pitch_of, gap, base, ppitch_of, pbase, vec = layout
    rng = np.random.default_rng(W * 131 + H + len(name))
    clip = _noise(rng, 6, H, W)
    pitch = pitch_of(W)
    # n = 1 with a previous frame, n = 2, n = 5 with and without one
    for n, with_prev in ((1, True), (2, False), (5, True), (5, False)):
        frames, prev = clip[1:1 + n], (clip[0] if with_prev else None)
        want = sr.frame_sums(frames, prev)
        expect = vec
        if name == "contiguous":
            expect = (3 * W) % 16 == 0 and (n == 1 or (H * pitch) % 16 == 0)
        if name == "odd_prev":
            expect = not with_prev
        if name == "gapped" and n == 1:
            expect = True                                # one frame: the stride is not used
        for order in (0, 1):
            f = frames[..., ::-1] if order else frames
            p = None if prev is None else (prev[..., ::-1] if order else prev)
            got = _run(env, f, p, pitch=pitch, stride=H * pitch + gap, base=base, prev_pitch=ppitch_of(W), prev_base=pbase, order=order, vec=expect)
            assert got == want, (name, n, with_prev, order)


def test_padding_is_not_read(env):
    """Two poisons: a sum that depended on a byte beyond 3 * width of a row would differ."""
    rng = np.random.default_rng(9)
    clip = _noise(rng, 4, 6, 36)
    want = sr.frame_sums(clip[1:], clip[0])
    for pitch, vec in ((128, True), (3 * 36 + 7, False)):
        for poison in (0x00, 0xFF, 0x5A):
            assert _run(env, clip[1:], clip[0], pitch=pitch, stride=6 * pitch + 32 * vec + 3 * (not vec), vec=vec, poison=poison) == want
    for factor in (2, 3):
        want = sr.frame_sums(clip[1:], clip[0], factor=factor)
        for poison in (0x00, 0xFF):
            assert _run(env, clip[1:], clip[0], pitch=128, factor=factor, vec=False, poison=poison) == want


def test_more_than_one_workgroup_and_row_tails(env):
    """200 x 70: 13 groups per row, the last of 8 pixels, 910 groups in 4 workgroups; the pixel kernel takes 55 workgroups."""
    rng = np.random.default_rng(21)
    clip = _noise(rng, 3, 70, 200)
    want = sr.frame_sums(clip)
    assert _run(env, clip, pitch=608, vec=True) == want
    assert _run(env, clip, pitch=601, vec=False) == want


FACTORS = [(36, 6, 2, "box"), (70, 21, 3, "linear"), (70, 21, 7, "linear"), (35, 7, 2, "odd: round(17.5) = 18, round(3.5) = 4")]


@pytest.mark.parametrize("W,H,factor,what", FACTORS, ids=[f"{w}x{h}_f{f}" for w, h, f, _ in FACTORS])
def test_factors(env, W, H, factor, what):
    rng = np.random.default_rng(W + factor)
    clip = _noise(rng, 5, H, W)
    for order in (0, 1):
        f = clip[..., ::-1] if order else clip
        assert _run(env, f[1:], f[0], order=order, factor=factor, vec=False) == sr.frame_sums(clip[1:], clip[0], factor=factor)
        assert _run(env, f, order=order, factor=factor, pitch=_up16(3 * W) + 16, vec=False) == sr.frame_sums(clip, factor=factor)


def test_auto_factor_of_a_512_wide_frame(env):
    from metric_depth_video_toolbox_amd import scene_detect as sd
    rng = np.random.default_rng(512)
    clip = _noise(rng, 3, 8, 512)
    factor = sd.downscale_factor("auto", 512, 8)
    assert factor == 2 == sr.auto_factor(512)
    assert _run(env, clip, factor=factor) == sr.frame_sums(clip, factor=2)


def test_contents(env):
    rng = np.random.default_rng(77)
    W, H = 36, 6
    same = np.repeat(_noise(rng, 1, H, W), 4, axis=0)
    grey = np.repeat(rng.integers(0, 256, (4, H, W, 1), dtype=np.uint8), 3, axis=3)
    # the six saturated primaries and their ties (v == r == g, v == g == b, v == r == b), dimmed too: every hue branch and the wrap
    cols = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [200, 200, 50], [10, 180, 180],
                     [220, 20, 220], [90, 30, 31], [31, 30, 90], [255, 255, 255], [0, 0, 0], [1, 0, 1], [254, 255, 254], [129, 128, 0]], np.uint8)
    prim = cols[rng.integers(0, len(cols), (4, H, W))]
    prim[0].reshape(-1, 3)[:len(cols)] = cols
    prim[1].reshape(-1, 3)[:len(cols)] = cols[::-1]
    for name, clip in (("same", same), ("grey", grey), ("primaries", prim)):
        want = sr.frame_sums(clip)
        if name == "same":
            assert want == [[0, 0, 0]] * 3
        if name == "grey":
            assert all(w[0] == 0 and w[1] == 0 and w[2] > 0 for w in want)
        if name == "primaries":
            assert all(min(w) > 0 for w in want)
        for pitch, vec in ((3 * W, False), (112, True)):
            for order in (0, 1):
                f = clip[..., ::-1] if order else clip
                assert _run(env, f, pitch=pitch, order=order, vec=vec) == want, (name, pitch, order)
                assert _run(env, f[1:], f[0], pitch=pitch, order=order, vec=vec) == want, (name, pitch, order)


def test_sums_beyond_32_bits(env):
    """4096 x 4128 = 16 908 288 pixels: 255 * pixels = 4 311 613 440 > 2^32.  White against black: V alone; (255, 0, 0) against black:
    S and V.  The frames are made on the device; the expected sums are the definition's."""
    torch, L, ctx = env
    W, H = 4096, 4128
    px = W * H
    assert 255 * px > 1 << 32
    frames = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    frames[1] = 255
    sums = torch.full((3 + 2,), -1, dtype=torch.int64, device="cuda")
    assert L.mdvt_scene_vector_path(2, frames.data_ptr(), 3 * W, 3 * W * H, None, 0, 1) == 1
    rc = L.mdvt_scene_frame_sums(ctx.handle, W, H, 2, frames.data_ptr(), 3 * W, 3 * W * H, 0, None, 0, 1, sums.data_ptr() + 8, None)
    assert rc == 0, L.mdvt_last_error(ctx.handle)
    assert sums.cpu().tolist() == [-1, 0, 0, 255 * px, -1]
    frames[1, :, :, 1:] = 0                              # (255, 0, 0); as B, G, R it is blue: the same S and V
    for order in (0, 1):
        sums.fill_(-1)
        # the byte path: the red frame alone from its second pixel on (an odd address), black as the previous frame
        assert L.mdvt_scene_vector_path(1, frames[1].data_ptr() + 3, 3 * W, 0, frames[0].data_ptr(), 3 * W, 1) == 0
        rc = L.mdvt_scene_frame_sums(ctx.handle, W - 1, H, 1, frames[1].data_ptr() + 3, 3 * W, 0, order, frames[0].data_ptr(), 3 * W, 1,
                                     sums.data_ptr() + 8, None)
        assert rc == 0, L.mdvt_last_error(ctx.handle)
        got = sums.cpu().tolist()
        hue, part = (120 if order else 0), (W - 1) * H
        assert 255 * part > 1 << 32
        assert got == [-1, hue * part, 255 * part, 255 * part, -1]
    sums.fill_(-1)
    rc = L.mdvt_scene_frame_sums(ctx.handle, W, H, 2, frames.data_ptr(), 3 * W, 3 * W * H, 0, None, 0, 1, sums.data_ptr() + 8, None)
    assert rc == 0, L.mdvt_last_error(ctx.handle)
    assert sums.cpu().tolist() == [-1, 0, 255 * px, 255 * px, -1]


REFUSALS = [
    ("null frames", dict(null="frames"), INVALID, "NULL buffer"),
    ("null sums", dict(null="sums"), INVALID, "NULL buffer"),
    ("misaligned sums", dict(sums_off=4), INVALID, "d_sums must be 8-byte aligned"),
    ("pitch", dict(pitch=3 * 36 - 1), INVALID, "pitch smaller than one row"),
    ("prev_pitch", dict(prev_pitch=3 * 36 - 1), INVALID, "prev_pitch smaller than one row"),
    ("stride", dict(stride=6 * 112 - 1), INVALID, "stride smaller than one frame"),
    ("n_frames 0", dict(n=0), INVALID, "n_frames must be >= 1"),
    ("n_frames -1", dict(n=-1), INVALID, "n_frames must be >= 1"),
    ("no pair", dict(n=1, no_prev=True), INVALID, "no pair to compare"),
    ("factor 0", dict(factor=0), INVALID, "factor must be >= 1"),
    ("factor -2", dict(factor=-2), INVALID, "factor must be >= 1"),
    ("factor leaves no row", dict(factor=13), INVALID, "factor 13 leaves a 3 x 0 image of a 36 x 6 frame"),
    ("order", dict(order=2), INVALID, "order must be 0 (RGB) or 1 (BGR), got 2"),
    ("width 0", dict(width=0), INVALID, "bad size 0 x 6"),
    ("too large", dict(width=1 << 14, height=(1 << 14) + 1, pitch=3 << 14, prev_pitch=3 << 14, stride=(3 << 14) * ((1 << 14) + 1)), UNSUPPORTED, "frame too large"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_arena_untouched(env, case):
    torch, L, ctx = env
    _, ch, code, text = case
    rng = np.random.default_rng(1)
    clip = _noise(rng, 4, 6, 36)
    a = Arena(torch, clip[1:], clip[0], 112, 6 * 112, 0, 112, 0)
    args = a.args()
    if ch.get("null") == "frames":
        args[3] = None
    if ch.get("null") == "sums":
        args[10] = None
    if "sums_off" in ch:
        args[10] += ch["sums_off"]
    for key, at in (("width", 0), ("height", 1), ("n", 2), ("pitch", 4), ("stride", 5), ("order", 6), ("prev_pitch", 8), ("factor", 9)):
        if key in ch:
            args[at] = ch[key]
    if ch.get("no_prev"):
        args[7], args[8] = None, 0
    rc = L.mdvt_scene_frame_sums(ctx.handle, *args, None)
    got = (L.mdvt_last_error(ctx.handle) or b"").decode()
    assert rc == code and text in got, (rc, got)
    assert a.untouched(torch)
    # the context is usable afterwards
    rc, got = _call(env, a)
    assert rc == 0, got
    assert a.sums(torch) == sr.frame_sums(clip[1:], clip[0])
