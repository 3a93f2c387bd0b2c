"""The four entry points of include/mdvt_infill_adapter.h through the raw C ABI and their Python faces in stereo_crafter_infill,
bit for bit against the NumPy restatement of tests/infill_adapter_ref.py (whose lower-side marks are the C oracle's and whose
dilation is SciPy's): up- and down-scaling with non-integer ratios, the copy and the 2 x 2 area path, widths around 4, 16 and 64,
padded pitches and strides, one frame and five; masks without holes, all holes, marks within 7 pixels of every border, mask
colours whose direction leaves the image.  Moments against Python integers; the colour match on the reference's own outputs
(tests/golden/lhm_transfer_*.npz) under the conditions of tests/test_infill_adapter_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import infill_adapter_ref as R

pytestmark = pytest.mark.gpu

GOLDENS = R.GOLDENS

POISON = 0xA5


class Buf:
    """`rows` rows of `row_bytes` bytes per frame in device memory with padded pitch and stride, poisoned; .get() -> the payload."""

    def __init__(self, n, rows, row_bytes, pad=0, spad=0, data=None, poison=POISON):
        import torch
        self.n, self.rows, self.row_bytes = n, rows, row_bytes
        self.pitch = row_bytes + pad
        self.stride = rows * self.pitch + spad
        self.host = np.full((n, self.stride), poison, dtype=np.uint8)
        if data is not None:
            self.view(self.host)[...] = np.ascontiguousarray(data).reshape(n, rows, -1).view(np.uint8)
        self.t = torch.from_numpy(self.host.copy()).cuda()
        self.ptr = C.c_void_p(self.t.data_ptr())

    def view(self, host):
        return host[:, :self.rows * self.pitch].reshape(self.n, self.rows, self.pitch)[:, :, :self.row_bytes]

    def get(self):
        self.after = self.t.cpu().numpy()
        return self.view(self.after)

    def padding_untouched(self):
        a, b = self.after.copy(), self.host.copy()
        self.view(a)[...] = 0
        self.view(b)[...] = 0
        return np.array_equal(a, b)


@pytest.fixture(scope="module")
def lib():
    import torch
    torch.cuda.init()
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    yield _lib.load(), ctx
    ctx.close()


def run_prepare(lib, color, mask, eye, mw, mh, pads=(0, 0)):
    L, ctx = lib
    n, H, W2 = color.shape[:3]
    pad, spad = pads
    bc, bm = Buf(n, H, 3 * W2, pad, spad, color), Buf(n, H, 3 * W2, pad + 1 if pad else 0, spad, mask)
    bi, bk = Buf(n, mh, 3 * mw, pad, spad), Buf(n, mh, mw, pad, 3 * spad)
    bh = Buf(1, 1, 4 * n)
    ctx.check(L.mdvt_adapter_prepare_eye(ctx.handle, W2 // 2, H, n, eye, bc.ptr, bc.pitch, bc.stride, bm.ptr, bm.pitch, bm.stride, mw, mh,
                                         bi.ptr, bi.pitch, bi.stride, bk.ptr, bk.pitch, bk.stride, bh.ptr, None))
    image, mmask = bi.get().reshape(n, mh, mw, 3).copy(), bk.get().reshape(n, mh, mw).copy()
    counts = bh.get().copy().view(np.uint32).reshape(n)
    assert bi.padding_untouched() and bk.padding_untouched()
    return image, mmask, counts


def run_composite(lib, model, color, mask, eye, pads=(0, 0)):
    L, ctx = lib
    n, H, W2 = color.shape[:3]
    mh, mw = model.shape[1:3]
    pad, spad = pads
    bc, bm = Buf(n, H, 3 * W2, pad, spad, color), Buf(n, H, 3 * W2, 2 * pad, spad, mask)
    bf = Buf(n, mh, 3 * mw, pad, spad, model)
    bp, bb = Buf(n, H, 3 * W2, pad, spad), Buf(n, H, 3 * W2, 3 * pad, 2 * spad, poison=0x5A)
    ctx.check(L.mdvt_adapter_composite_eye(ctx.handle, W2 // 2, H, n, eye, bf.ptr, mw, mh, bf.pitch, bf.stride, bc.ptr, bc.pitch, bc.stride,
                                           bm.ptr, bm.pitch, bm.stride, bp.ptr, bp.pitch, bp.stride, bb.ptr, bb.pitch, bb.stride, None))
    pasted, blended = bp.get().reshape(n, H, W2, 3).copy(), bb.get().reshape(n, H, W2, 3).copy()
    assert bp.padding_untouched() and bb.padding_untouched()
    other = 1 - eye
    assert (R.eye_of(pasted, other) == POISON).all() and (R.eye_of(blended, other) == 0x5A).all(), "the other eye's half was written"
    return R.eye_of(pasted, eye), R.eye_of(blended, eye)


# eye (w, h) -> model (w, h): up and down with non-integer ratios, the copy, the exact half, one axis equal
SIZES = [((37, 23), (64, 48)), ((37, 23), (40, 24)), ((64, 48), (64, 48)), ((64, 48), (40, 24)), ((80, 48), (40, 24)), ((64, 23), (64, 48))]
KINDS = ("none", "all", "border", "mixed")


@pytest.mark.parametrize("case", range(len(SIZES)))
def test_prepare_and_composite_equal_the_restatement(lib, orc, case):
    (ew, eh), (mw, mh) = SIZES[case]
    rng = np.random.default_rng(100 + case)
    for k, kind in enumerate(KINDS):
        n = (1, 5)[(case + k) % 2]
        pads = ((0, 0), (5, 64), (3, 7))[(case + k) % 3]
        color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
        mask = R.make_masks(rng, n, eh, ew, kind)
        for eye in (0, 1):
            tag = f"eye {eye} {ew}x{eh} -> {mw}x{mh} n={n} {kind} pads={pads}"
            image, mmask, counts = run_prepare(lib, color, mask, eye, mw, mh, pads)
            wi, wm, wc = R.prepare_eye(color, mask, eye, mw, mh)
            assert np.array_equal(image, wi), tag
            assert np.array_equal(mmask, wm), tag
            assert np.array_equal(counts, wc), f"{tag}: hole counts {counts} vs {wc}"
            if kind == "none":
                assert not counts.any()
            if kind == "all":
                assert (counts == mw * mh).all()
            model = rng.integers(0, 256, (n, mh, mw, 3), dtype=np.uint8)      # (any frames will do: the model's output is arbitrary)
            pasted, blended = run_composite(lib, model, color, mask, eye, pads)
            wp, wb = R.composite_eye(model, color, mask, eye, orc)
            assert np.array_equal(pasted, wp), tag
            bad = np.argwhere(blended != wb)
            assert len(bad) == 0, f"{tag}: {len(bad)} blended bytes differ, first {bad[:4].tolist()}"
            if kind == "border":                                              # the test is worth its name: the alpha reaches every border
                a = R.alpha_of(R.eye_of(mask[0], eye), orc)[0]
                assert a[0].max() > 0 and a[-1].max() > 0 and a[:, 0].max() > 0 and a[:, -1].max() > 0, tag


@pytest.mark.parametrize("ew", [3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_prepare_widths_around_the_vector_sizes(lib, ew):
    rng = np.random.default_rng(ew)
    n, eh, (mw, mh) = 2, 9, (21, 13)
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, "mixed")
    for eye in (0, 1):
        image, mmask, counts = run_prepare(lib, color, mask, eye, mw, mh, (ew % 3, ew % 5))
        wi, wm, wc = R.prepare_eye(color, mask, eye, mw, mh)
        assert np.array_equal(image, wi) and np.array_equal(mmask, wm) and np.array_equal(counts, wc), (ew, eye)


@pytest.mark.parametrize("ew", [8, 15, 16, 17, 63, 65])
def test_composite_widths_around_the_vector_sizes(lib, orc, ew):
    rng = np.random.default_rng(50 + ew)
    n, eh, (mw, mh) = 2, 11, (24, 16)
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, "mixed" if ew % 2 else "border")
    model = rng.integers(0, 256, (n, mh, mw, 3), dtype=np.uint8)
    for eye in (0, 1):
        pasted, blended = run_composite(lib, model, color, mask, eye, (ew % 4, 0))
        wp, wb = R.composite_eye(model, color, mask, eye, orc)
        assert np.array_equal(pasted, wp) and np.array_equal(blended, wb), (ew, eye)


def test_composite_refuses_small_eyes_and_bad_layouts(lib):
    L, ctx = lib
    b = Buf(1, 16, 3 * 32)
    o1, o2 = Buf(1, 16, 3 * 32), Buf(1, 16, 3 * 32)

    def call(ew=16, eh=16, n=1, eye=0, pitch=96, model=b.ptr):
        return L.mdvt_adapter_composite_eye(ctx.handle, ew, eh, n, eye, model, 8, 8, 24, 0, b.ptr, pitch, 0, b.ptr, pitch, 0,
                                            o1.ptr, pitch, 0, o2.ptr, pitch, 0, None)
    assert call(ew=7) == -3 and call(eh=7) == -3                    # MDVT_ERR_UNSUPPORTED
    assert call(eye=2) == -1 and call(pitch=95) == -1 and call(n=0) == -1 and call(model=None) == -1 and call(ew=0) == -1
    assert (o1.get() == POISON).all() and (o2.get() == POISON).all()


# ---- moments and the colour match -------------------------------------------------------------------------------------------------

def run_moments(lib, frames, mask=None, pads=(0, 0)):
    L, ctx = lib
    n, H, W = frames.shape[:3]
    bf = Buf(n, H, 3 * W, pads[0], pads[1], frames)
    bm = Buf(n, H, W, pads[0], pads[1], mask) if mask is not None else None
    bo = Buf(1, 1, 80 * n)
    ctx.check(L.mdvt_lhm_moments(ctx.handle, W, H, n, bf.ptr, bf.pitch, bf.stride, bm.ptr if bm else None, bm.pitch if bm else 0,
                                 bm.stride if bm else 0, bo.ptr, None))
    return [[int(v) for v in row] for row in bo.get().copy().view(np.uint64).reshape(n, 10)]


def test_moments_of_a_white_frame_pass_2_to_the_32(lib):
    frames = np.full((1, 768, 1024, 3), 255, dtype=np.uint8)
    npx = 768 * 1024
    want = [[npx] + [255 * npx] * 3 + [255 * 255 * npx] * 6]
    assert want[0][4] > 1 << 32
    assert run_moments(lib, frames) == want
    assert run_moments(lib, frames, pads=(1, 0)) == want            # the byte path (pitch not a multiple of 4)


def test_moments_widen_before_a_lane_passes_65536_pixels(lib):
    """One row of 2^24 + 4101 white pixels: one workgroup, each lane more than 65536 pixels (65537 * 255^2 > 2^32)."""
    W = (1 << 24) + 4101
    frames = np.full((1, 1, W, 3), 255, dtype=np.uint8)
    want = [[W] + [255 * W] * 3 + [255 * 255 * W] * 6]
    assert W / 256 > 65536
    assert run_moments(lib, frames) == want                         # (W * 3 is odd: the byte path)
    assert run_moments(lib, frames, pads=(1, 0)) == want            # pitch a multiple of 4: the dword path


@pytest.mark.parametrize("case", range(6))
def test_moments_equal_python_integers(lib, case):
    rng = np.random.default_rng(300 + case)
    n, H, W = ((1, 7, 5), (5, 23, 37), (2, 48, 64), (3, 9, 258), (2, 300, 17), (1, 2, 1030))[case]
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    mask = (rng.random((n, H, W)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (n, H, W), dtype=np.uint8)
    for pads in ((0, 0), (1, 3), (4, 8)):
        assert run_moments(lib, frames, None, pads) == R.moments(frames), (case, pads)
        assert run_moments(lib, frames, mask, pads) == R.moments(frames, mask), (case, pads)


def test_moments_with_masks_that_keep_0_2_and_3_pixels(lib):
    z = np.load(os.path.join(os.path.dirname(GOLDENS[0]), "lhm_transfer_few_kept.npz"))
    got = run_moments(lib, z["reference"], z["mask"])
    assert [g[0] for g in got] == [0, 2, 3] and got[0] == [0] * 10
    assert got == R.moments(z["reference"], z["mask"])


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[13:-4] for p in GOLDENS])
def test_colour_match_on_the_goldens(lib, path):
    """The Python face (moments -> host algebra -> apply, one read-back) on the reference's inputs: the restatement's bytes, and the
    reference's float64 output under the conditions of the CPU test."""
    import torch
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    z = np.load(path)
    video, reference, mask = (torch.from_numpy(z[k]).cuda() for k in ("video", "reference", "mask"))
    got = sci.transfer_lhm_video_refmask(video, reference, mask).cpu().numpy()
    assert np.array_equal(got, R.transfer_lhm(z["video"], z["reference"], z["mask"]))
    R.check_against_golden(got, z, os.path.basename(path))
    # the raw call with padded rows, one frame's parameters at a time and all at once
    L, ctx = lib
    mx, mr, ma = R.moments(z["video"]), R.moments(z["reference"], z["mask"]), R.moments(z["reference"])
    params = np.array([R.lhm_params(mx[k], mr[k], ma[k]) for k in range(len(mx))])
    n, H, W = z["video"].shape[:3]
    for pads in ((0, 0), (2, 5), (4, 12)):
        bi, bo, bp = Buf(n, H, 3 * W, pads[0], pads[1], z["video"]), Buf(n, H, 3 * W, pads[0], pads[1]), Buf(1, 1, 120 * n, data=params.view(np.uint8))
        ctx.check(L.mdvt_lhm_apply(ctx.handle, W, H, n, bi.ptr, bi.pitch, bi.stride, bp.ptr, bo.ptr, bo.pitch, bo.stride, None))
        assert np.array_equal(bo.get().reshape(n, H, W, 3), got) and bo.padding_untouched(), pads


def test_python_faces_on_strided_views(lib, orc):
    """prepare_eye / composite_eye of stereo_crafter_infill on tensors as process_pair hands them over."""
    import torch
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    rng = np.random.default_rng(9)
    n, eh, ew, size = 5, 23, 37, (40, 24)
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, "mixed")
    d_color, d_mask = torch.from_numpy(color).cuda(), torch.from_numpy(mask).cuda()
    pasted, blended = torch.zeros_like(d_color), torch.zeros_like(d_color)
    for eye in (0, 1):
        image, mmask, counts = sci.prepare_eye(d_color, d_mask, eye, size)
        wi, wm, wc = R.prepare_eye(color, mask, eye, *size)
        assert np.array_equal(image.cpu().numpy(), wi) and np.array_equal(mmask.cpu().numpy(), wm) and np.array_equal(counts.cpu().numpy(), wc.astype(np.int32))
        sci.composite_eye(image[1:4], d_color[1:4], d_mask[1:4], eye, pasted[1:4], blended[1:4])
        wp, wb = R.composite_eye(wi[1:4], color[1:4], mask[1:4], eye, orc)
        assert np.array_equal(R.eye_of(pasted.cpu().numpy()[1:4], eye), wp) and np.array_equal(R.eye_of(blended.cpu().numpy()[1:4], eye), wb)
    assert not pasted[0].any() and not blended[4].any()
