"""mdvt_inspatio_prepare_eye and mdvt_inspatio_model_frames (include/mdvt_inspatio.h) through the raw C ABI against
tests/inspatio_ref.py, bit for bit: inputs and outputs inside one arena of pseudo-random poison (and, again, of its complement), of
which only the outputs' own row bytes and the hole counts may change."""
import numpy as np
import pytest

import infill_adapter_ref as iar
import inspatio_ref as ir

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
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
    """Regions of rows: name -> (n, rows, row bytes, pitch, stride, offset); inputs are filled, outputs read back."""

    def __init__(self, torch, regions, pad=0, gap=0, base=0, flip=False, seed=5):
        self.torch, self.at, at = torch, {}, MARGIN
        for name, (n, rows, width, data) in regions.items():
            pitch = width + pad
            stride = rows * pitch + gap
            self.at[name] = (n, rows, width, pitch, stride, at + base)
            at = _up(at + base + n * stride + MARGIN)
        self.at_holes = at
        n0 = next(iter(regions.values()))[0]
        total = at + 4 * n0 + MARGIN
        poison = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
        self.buf = torch.from_numpy(~poison if flip else poison).cuda()
        for name, (n, rows, width, data) in regions.items():
            if data is not None:
                _, _, _, pitch, stride, off = self.at[name]
                torch.as_strided(self.buf, (n, rows, width), (stride, pitch, 1), off).copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(n, rows, width)).cuda())
        self.before = self.buf.cpu().numpy().copy()
        self.ptr, self.outs, self.n = self.buf.data_ptr(), [k for k, v in regions.items() if v[3] is None], n0

    def triple(self, name):
        _, _, _, pitch, stride, off = self.at[name]
        return [self.ptr + off, pitch, stride]

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.buf.cpu().numpy() == self.before).all())

    def read(self, holes=True):
        self.torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        keep, out = np.ones(len(got), bool), {}
        for name in self.outs:
            n, rows, width, pitch, stride, off = self.at[name]
            img = np.zeros((n, rows, width), np.uint8)
            for k in range(n):
                for y in range(rows):
                    a = off + k * stride + y * pitch
                    keep[a:a + width] = False
                    img[k, y] = got[a:a + width]
            out[name] = img
        if holes:
            keep[self.at_holes:self.at_holes + 4 * self.n] = False
            out["holes"] = got[self.at_holes:self.at_holes + 4 * self.n].copy().view(np.uint32).tolist()
        assert (got[keep] == self.before[keep]).all(), "bytes outside the outputs changed"
        return out


def _clip(rng, n, H, W):
    """Side-by-side colour and mask frames [n, H, 2 W, 3]: rectangular holes, isolated mask pixels with one non-zero channel."""
    color = rng.integers(0, 256, (n, H, 2 * W, 3), dtype=np.uint8)
    mask = np.zeros_like(color)
    for k in range(n):
        for _ in range(6):
            y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, 2 * W - 4))
            mask[k, y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 9))] = 255
        for c in range(3):
            for _ in range(3):
                mask[k, int(rng.integers(0, H)), int(rng.integers(0, 2 * W)), c] = int(rng.integers(1, 256))
    mask[0, 0, :] = 255                                             # holes on the border
    mask[0, :, 2 * W - 1] = 255
    return color, mask


def _prepare(env, color, mask, eye, mw, mh, **layout):
    torch, L, ctx = env
    n, H, W2, _ = color.shape
    W = W2 // 2
    a = Arena(torch, dict(color=(n, H, 6 * W, color), mask=(n, H, 6 * W, mask), valid=(n, H, W, None), render=(n, H, 3 * W, None),
                          mvalid=(n, mh, mw, None), mrender=(n, mh, 3 * mw, None)), **layout)
    args = [W, H, n, eye, *a.triple("color"), *a.triple("mask"), mw, mh, *a.triple("valid"), *a.triple("render"), *a.triple("mvalid"),
            *a.triple("mrender"), a.ptr + a.at_holes]
    return a, args


SIZES = [(41, 33, 41, 33, "equal size"), (64, 40, 32, 20, "exact 2 x"), (41, 33, 52, 30, "linear"), (90, 46, 26, 15, "linear, reduced")]


@pytest.mark.parametrize("W,H,mw,mh,what", SIZES, ids=[s[4] for s in SIZES])
def test_prepare_eye_equals_the_restatement(env, W, H, mw, mh, what):
    torch, L, ctx = env
    rng = np.random.default_rng(W * H + mw)
    color, mask = _clip(rng, 3, H, W)
    for eye in (0, 1):
        want = [ir.prepare_eye(color[k], mask[k], eye, mw, mh) for k in range(3)]
        assert all(w[4] > 0 for w in want) and any((w[2] % 255 != 0).any() for w in want) == (what != "equal size"), "the plane is not thresholded"
        for n, layout in ((3, dict()), (3, dict(pad=5, gap=7, base=3)), (1, dict(pad=16))):
            for flip in (False, True):
                a, args = _prepare(env, color[:n], mask[:n], eye, mw, mh, flip=flip, **layout)
                rc = L.mdvt_inspatio_prepare_eye(ctx.handle, *args, None)
                assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
                got = a.read()
                assert got["holes"] == [w[4] for w in want[:n]]
                for name, k in (("valid", 0), ("render", 1), ("mvalid", 2), ("mrender", 3)):
                    assert np.array_equal(got[name], np.stack([w[k].reshape(w[k].shape[0], -1) for w in want[:n]])), (name, eye, n, flip)


def test_an_eye_without_holes_counts_zero(env):
    torch, L, ctx = env
    rng = np.random.default_rng(6)
    color, mask = _clip(rng, 2, 20, 24)
    mask[1, :, :24] = 0
    a, args = _prepare(env, color, mask, 0, 12, 10)
    assert L.mdvt_inspatio_prepare_eye(ctx.handle, *args, None) == 0
    got = a.read()
    assert got["holes"][1] == 0 and got["holes"][0] > 0 and (got["valid"][1] == 255).all() and np.array_equal(got["render"][1].reshape(20, 24, 3), color[1, :, :24])


@pytest.mark.parametrize("W,H,mw,mh,what", SIZES, ids=[s[4] for s in SIZES])
def test_model_frames_equals_the_u8_resize(env, W, H, mw, mh, what):
    torch, L, ctx = env
    rng = np.random.default_rng(W + H)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    want = np.stack([iar.resize_u8(f, mw, mh).reshape(mh, 3 * mw) for f in frames])
    for layout in (dict(), dict(pad=7, gap=5, base=1)):
        for flip in (False, True):
            a = Arena(torch, dict(frames=(2, H, 3 * W, frames), out=(2, mh, 3 * mw, None)), flip=flip, **layout)
            rc = L.mdvt_inspatio_model_frames(ctx.handle, W, H, 2, *a.triple("frames"), mw, mh, *a.triple("out"), None)
            assert rc == 0, (L.mdvt_last_error(ctx.handle) or b"").decode()
            assert np.array_equal(a.read(holes=False)["out"], want)


REFUSALS = [
    ("null color", {4: None}, INVALID, "NULL buffer"), ("null mask", {7: None}, INVALID, "NULL buffer"), ("null valid", {12: None}, INVALID, "NULL buffer"),
    ("null counts", {24: None}, INVALID, "NULL buffer"), ("eye 2", {3: 2}, INVALID, "eye must be 0 (left half) or 1 (right half), got 2"),
    ("width 0", {0: 0}, INVALID, "bad size"), ("model height 0", {11: 0}, INVALID, "bad size"), ("n_frames 0", {2: 0}, INVALID, "n_frames must be >= 1"),
    ("color pitch", {5: 6 * 24 - 1}, INVALID, "pitch smaller than one side-by-side row"), ("mask pitch", {8: 6 * 24 - 1}, INVALID, "pitch smaller than one side-by-side row"),
    ("valid pitch", {13: 23}, INVALID, "output pitch smaller than one row"), ("model render pitch", {22: 35}, INVALID, "output pitch smaller than one row"),
    ("render stride", {17: 20 * 72 - 1}, INVALID, "stride smaller than one frame"), ("model valid stride", {20: 119}, INVALID, "stride smaller than one frame"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_arena_untouched(env, case):
    torch, L, ctx = env
    _, change, code, text = case
    rng = np.random.default_rng(9)
    color, mask = _clip(rng, 2, 20, 24)
    a, args = _prepare(env, color, mask, 1, 12, 10)
    bad = list(args)
    for at, v in change.items():
        bad[at] = v
    rc = L.mdvt_inspatio_prepare_eye(ctx.handle, *bad, None)
    got = (L.mdvt_last_error(ctx.handle) or b"").decode()
    assert rc == code and text in got, (rc, got)
    assert a.untouched()
    assert L.mdvt_inspatio_prepare_eye(ctx.handle, *args, None) == 0
    assert a.read()["holes"] == [ir.prepare_eye(color[k], mask[k], 1, 12, 10)[4] for k in range(2)]
    misaligned = list(args)
    misaligned[24] += 2
    assert L.mdvt_inspatio_prepare_eye(ctx.handle, *misaligned, None) == INVALID
