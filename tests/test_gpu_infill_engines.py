"""The two entry points of include/mdvt_infill_engines.h through the raw C ABI and their Python faces in m2svid_infill and
stereo_dissoclusion_net_infill, bit for bit against tests/infill_engines_ref.py: the m2svid inputs against the NumPy restatement of the
u8 resize (up- and down-scaling, the copy, the 2 x 2 area path, masks smaller and larger than the eye, an original frame of another
size), the finish against the plain-C oracle's own stages composed in Python.  Padded pitches and strides, one image and five."""
import ctypes as C

import numpy as np
import pytest

import infill_adapter_ref as R
import infill_engines_ref as E

pytestmark = pytest.mark.gpu

POISON = 0xA5
INVALID, UNSUPPORTED = -1, -3


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

    def untouched(self):
        return np.array_equal(self.t.cpu().numpy(), self.host)

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


# ---- mdvt_m2svid_prepare_eye ------------------------------------------------------------------------------------------------------

def run_prepare(lib, color, mask, org, eye, image_size, mask_size, pads=(0, 0)):
    L, ctx = lib
    n, H, W2 = color.shape[:3]
    oh, ow = org.shape[1:3]
    (iw, ih), (mw, mh) = image_size, mask_size
    pad, spad = pads
    bc, bm = Buf(n, H, 3 * W2, pad, spad, color), Buf(n, H, 3 * W2, pad + 1 if pad else 0, spad, mask)
    bo = Buf(n, oh, 3 * ow, 2 * pad, spad, org)
    bi, bg, bk = Buf(n, ih, 3 * iw, pad, spad), Buf(n, ih, 3 * iw, 3 * pad, 2 * spad, poison=0x5A), Buf(n, mh, mw, pad, 3 * spad)
    bh = Buf(1, 1, 4 * n)                                           # the counts arrive poisoned
    ctx.check(L.mdvt_m2svid_prepare_eye(ctx.handle, W2 // 2, H, n, eye, bc.ptr, bc.pitch, bc.stride, bm.ptr, bm.pitch, bm.stride,
                                        bo.ptr, ow, oh, bo.pitch, bo.stride, iw, ih, mw, mh, bi.ptr, bi.pitch, bi.stride,
                                        bg.ptr, bg.pitch, bg.stride, bk.ptr, bk.pitch, bk.stride, bh.ptr, None))
    image, org_image = bi.get().reshape(n, ih, iw, 3).copy(), bg.get().reshape(n, ih, iw, 3).copy()
    mmask, counts = bk.get().reshape(n, mh, mw).copy(), bh.get().copy().view(np.uint32).reshape(n)
    assert bi.padding_untouched() and bg.padding_untouched() and bk.padding_untouched()
    assert bc.untouched() and bm.untouched() and bo.untouched()
    return image, org_image, mmask, counts


def check_prepare(lib, rng, n, ew, eh, org_size, image_size, mask_size, kind, pads, tag):
    ow, oh = org_size
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    org = rng.integers(0, 256, (n, oh, ow, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, kind)
    for eye in (0, 1):
        got = run_prepare(lib, color, mask, org, eye, image_size, mask_size, pads)
        want = E.m2s_prepare_eye(color, mask, org, eye, image_size, mask_size)
        for g, w, what in zip(got, want, ("image", "org_image", "mask", "counts")):
            assert np.array_equal(g, w), f"{tag} eye {eye}: {what} differs"
        if kind == "none":
            assert not got[3].any()
        if kind == "all":
            assert (got[3] == mask_size[0] * mask_size[1]).all()


# eye, image, mask, original (w, h each): up and down with non-integer ratios, the image equal to the eye and exactly half of it, masks
# smaller than the eye, larger, and larger in one axis only; the original of another size than the eye (once exactly twice the image)
PREPARE = [((37, 23), (64, 48), (8, 8), (50, 30)), ((37, 23), (40, 24), (5, 3), (29, 31)), ((64, 48), (64, 48), (64, 64), (128, 96)),
           ((64, 48), (40, 24), (8, 8), (40, 24)), ((80, 48), (40, 24), (5, 3), (33, 17)), ((64, 23), (64, 48), (64, 64), (80, 48)),
           ((37, 23), (64, 48), (64, 64), (36, 22)), ((64, 48), (32, 24), (32, 24), (64, 47))]
KINDS = ("none", "all", "border", "mixed")


@pytest.mark.parametrize("case", range(len(PREPARE)))
def test_prepare_equals_the_restatement(lib, case):
    (ew, eh), image_size, mask_size, org_size = PREPARE[case]
    rng = np.random.default_rng(700 + case)
    for k, kind in enumerate(KINDS):
        n = (1, 5)[(case + k) % 2]
        pads = ((0, 0), (5, 64), (3, 7))[(case + k) % 3]
        check_prepare(lib, rng, n, ew, eh, org_size, image_size, mask_size, kind, pads,
                      f"{ew}x{eh} -> {image_size} / {mask_size}, org {org_size}, n={n} {kind} pads={pads}")


@pytest.mark.parametrize("ew", [3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_prepare_widths_around_the_vector_sizes(lib, ew):
    rng = np.random.default_rng(ew)
    check_prepare(lib, rng, 2, ew, 9, (ew + 2, 7), (21, 13), (6, 4), "mixed", (ew % 3, ew % 5), f"ew={ew}")


def test_prepare_at_the_real_size(lib):
    """A 960 x 1080 eye and a 1920 x 1080 original to 512 x 512 and 64 x 64, one frame."""
    rng = np.random.default_rng(960)
    check_prepare(lib, rng, 1, 960, 1080, (1920, 1080), (512, 512), (64, 64), "mixed", (0, 0), "real size")


def test_prepare_refusals_leave_the_outputs_untouched(lib):
    L, ctx = lib
    ew, eh, ow, oh, iw, ih, mw, mh = 16, 12, 20, 10, 8, 6, 4, 3
    src, org = Buf(2, eh, 6 * ew), Buf(2, oh, 3 * ow)
    outs = [Buf(2, ih, 3 * iw), Buf(2, ih, 3 * iw), Buf(2, mh, mw), Buf(1, 1, 8)]
    ok = dict(ctx=ctx.handle, ew=ew, eh=eh, n=2, eye=0, color=src.ptr, cp=src.pitch, cs=src.stride, mask=src.ptr, mp=src.pitch, ms=src.stride,
              org=org.ptr, ow=ow, oh=oh, op=org.pitch, os=org.stride, iw=iw, ih=ih, mw=mw, mh=mh,
              image=outs[0].ptr, ip=outs[0].pitch, is_=outs[0].stride, oimage=outs[1].ptr, oip=outs[1].pitch, ois=outs[1].stride,
              mmask=outs[2].ptr, kp=outs[2].pitch, ks=outs[2].stride, counts=outs[3].ptr)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mdvt_m2svid_prepare_eye(a["ctx"], a["ew"], a["eh"], a["n"], a["eye"], a["color"], a["cp"], a["cs"], a["mask"], a["mp"], a["ms"],
                                         a["org"], a["ow"], a["oh"], a["op"], a["os"], a["iw"], a["ih"], a["mw"], a["mh"], a["image"], a["ip"], a["is_"],
                                         a["oimage"], a["oip"], a["ois"], a["mmask"], a["kp"], a["ks"], a["counts"], None)
    bad = [dict(ctx=None)] + [{k: None} for k in ("color", "mask", "org", "image", "oimage", "mmask", "counts")]
    bad += [{k: 0} for k in ("ew", "eh", "n", "ow", "oh", "iw", "ih", "mw", "mh")] + [dict(eye=2), dict(eye=-1), dict(n=-1)]
    bad += [dict(cp=6 * ew - 1), dict(mp=6 * ew - 1), dict(op=3 * ow - 1), dict(ip=3 * iw - 1), dict(oip=3 * iw - 1), dict(kp=mw - 1)]
    bad += [dict(cs=eh * src.pitch - 1), dict(ms=eh * src.pitch - 1), dict(os=oh * org.pitch - 1), dict(is_=ih * 3 * iw - 1),
            dict(ois=ih * 3 * iw - 1), dict(ks=mh * mw - 1)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    assert call(n=1, ih=65536) == UNSUPPORTED and call(n=1, mh=65536) == UNSUPPORTED
    assert all(o.untouched() for o in outs)
    assert call(n=1, cs=0, ms=0, os=0, is_=0, ois=0, ks=0) == 0      # one frame: the strides do not matter
    assert call() == 0


# ---- mdvt_model_infill_finish ---------------------------------------------------------------------------------------------------

def run_finish(lib, img, model, mask, pads=(0, 0)):
    L, ctx = lib
    n, H, W = img.shape[:3]
    pad, spad = pads
    bi, bp, bm = Buf(n, H, 3 * W, pad, spad, img), Buf(n, H, 3 * W, 2 * pad, spad, model), Buf(n, H, 3 * W, pad + 1 if pad else 0, 2 * spad, mask)
    bo = Buf(n, H, 3 * W, 3 * pad, spad)
    ctx.check(L.mdvt_model_infill_finish(ctx.handle, W, H, n, bi.ptr, bi.pitch, bi.stride, bp.ptr, bp.pitch, bp.stride, bm.ptr, bm.pitch, bm.stride,
                                         bo.ptr, bo.pitch, bo.stride, None))
    out = bo.get().reshape(n, H, W, 3).copy()
    assert bo.padding_untouched() and bi.untouched() and bp.untouched() and bm.untouched()
    return out


def finish_inputs(rng, n, W, H, kinds):
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    model = (img.astype(np.int64) + rng.integers(1, 256, img.shape)).astype(np.uint8)       # differs from img in every byte
    assert (model != img).all()
    mask = np.array([E.finish_masks(rng, H, W, kinds[k % len(kinds)]) for k in range(n)])
    return img, model, mask


# around the 128 x 16 collecting tile
FINISH_SIZES = [(7, 5), (16, 9), (37, 23), (127, 15), (128, 16), (129, 17), (130, 33)]


@pytest.mark.parametrize("size", FINISH_SIZES, ids=[f"{w}x{h}" for w, h in FINISH_SIZES])
def test_finish_equals_the_composed_oracle(lib, orc, size):
    W, H = size
    rng = np.random.default_rng(1000 * W + H)
    for k, kind in enumerate(E.FINISH_KINDS):
        pads = ((0, 0), (5, 64), (3, 7), (4, 8))[(W + k) % 4]
        img, model, mask = finish_inputs(rng, 1, W, H, (kind,))
        got = run_finish(lib, img, model, mask, pads)
        want = E.finish(img, model, mask, orc)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{W}x{H} {kind} pads={pads}: {len(bad)} bytes differ, first {bad[:4].tolist()}"
        if kind == "none":
            assert np.array_equal(got, img)                        # an all-black mask: out == img
        if kind == "all":
            assert (got != img).any()
    # five images of assorted kinds in one call (W % 4 == 0 with tight rows: the dword path of the dense pass)
    img, model, mask = finish_inputs(rng, 5, W, H, E.FINISH_KINDS[1:])
    for pads in ((0, 0), (1, 3)):
        got = run_finish(lib, img, model, mask, pads)
        assert np.array_equal(got, E.finish(img, model, mask, orc)), f"{W}x{H} n=5 pads={pads}"


def test_finish_with_more_images_than_one_launch_set(lib, orc):
    rng = np.random.default_rng(17)
    img, model, mask = finish_inputs(rng, 19, 20, 11, E.FINISH_KINDS)
    assert np.array_equal(run_finish(lib, img, model, mask, (4, 4)), E.finish(img, model, mask, orc))


def test_finish_scratch_grows_with_a_larger_call(orc):
    """A fresh context: a small call, a larger one (the scratch block is replaced), the small size again (it is kept)."""
    import torch
    torch.cuda.init()
    from metric_depth_video_toolbox_amd import _lib
    ctx = _lib.Context(0, 16, 16)
    try:
        lib = (_lib.load(), ctx)
        rng = np.random.default_rng(23)
        seen = []
        for W, H, n in ((16, 9, 1), (130, 33, 5), (37, 23, 2), (130, 33, 5)):
            img, model, mask = finish_inputs(rng, n, W, H, ("mixed", "borders", "deep"))
            assert np.array_equal(run_finish(lib, img, model, mask), E.finish(img, model, mask, orc)), (W, H, n)
            seen.append(ctx.workspace_bytes())
        assert seen[1] > seen[0] and seen[2] == seen[1] == seen[3]
    finally:
        ctx.close()


def test_finish_refusals_leave_the_output_untouched(lib):
    L, ctx = lib
    W, H = 16, 12
    src, out = Buf(2, H, 3 * W), Buf(2, H, 3 * W)
    ok = dict(ctx=ctx.handle, W=W, H=H, n=2, img=src.ptr, ip=src.pitch, is_=src.stride, model=src.ptr, pp=src.pitch, ps=src.stride,
              mask=src.ptr, mp=src.pitch, ms=src.stride, out=out.ptr, op=out.pitch, os=out.stride)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mdvt_model_infill_finish(a["ctx"], a["W"], a["H"], a["n"], a["img"], a["ip"], a["is_"], a["model"], a["pp"], a["ps"],
                                          a["mask"], a["mp"], a["ms"], a["out"], a["op"], a["os"], None)
    bad = [dict(ctx=None)] + [{k: None} for k in ("img", "model", "mask", "out")] + [{k: 0} for k in ("W", "H", "n")] + [dict(n=-1)]
    bad += [{k: 3 * W - 1} for k in ("ip", "pp", "mp", "op")] + [{k: H * 3 * W - 1} for k in ("is_", "ps", "ms", "os")]
    bad += [dict(out=src.ptr)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    # the marches' limits: a mask pitch of 2^24, and pitch x height of 2^32 (nothing is read: the call is refused first)
    assert call(mp=1 << 24, ms=(1 << 24) * H) == UNSUPPORTED
    assert call(n=1, H=1 << 9, mp=1 << 23) == UNSUPPORTED
    assert call(n=1, H=65536) == UNSUPPORTED
    assert out.untouched()
    assert call(n=1, is_=0, ps=0, ms=0, os=0) == 0 and call() == 0


# ---- the Python faces -----------------------------------------------------------------------------------------------------------

def test_python_faces_on_strided_views(lib, orc):
    """prepare_eye of m2svid_infill and sdiss_infill / model_infill_finish of stereo_dissoclusion_net_infill on views of side-by-side
    tensors, as their process_pair hands them over."""
    import torch
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    rng = np.random.default_rng(9)
    n, eh, ew = 5, 23, 37
    color = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    org = rng.integers(0, 256, (n, 19, 31, 3), dtype=np.uint8)
    depth = rng.integers(0, 256, (n, eh, 2 * ew, 3), dtype=np.uint8)
    mask = R.make_masks(rng, n, eh, ew, "mixed")
    mask[mask.any(axis=-1) & (rng.random(mask.shape[:3]) < 0.8)] |= 1       # most hole pixels are bg too
    d_color, d_mask, d_org, d_depth = (torch.from_numpy(a).cuda() for a in (color, mask, org, depth))
    for eye in (0, 1):
        got = m2s.prepare_eye(d_color[1:4], d_mask[1:4], d_org[1:4], eye, (40, 24), (6, 5))
        want = E.m2s_prepare_eye(color[1:4], mask[1:4], org[1:4], eye, (40, 24), (6, 5))
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w.astype(np.int32) if w.dtype == np.uint32 else w)

    def gen_numpy(image, infill_mask, dep):
        return ((image.astype(np.int64) * 3 // 4 + 17 + (dep * np.float32(64)).astype(np.int64)[..., None]) % 256).astype(np.uint8)

    def gen_torch(image, infill_mask, dep):
        assert image.is_contiguous() and infill_mask.is_contiguous() and dep.is_contiguous() and dep.dtype == torch.float32
        assert image.shape == infill_mask.shape == dep.shape + (3,)
        return ((torch.div(image.to(torch.int64) * 3, 4, rounding_mode="floor") + 17 + (dep * 64).to(torch.int64)[..., None]) % 256).to(torch.uint8)
    d_out = torch.zeros_like(d_color)
    for eye in (0, 1):
        half = slice(eye * ew, (eye + 1) * ew)
        before = d_color.clone()
        sdn.sdiss_infill(d_color[1:4, :, half], d_mask[1:4, :, half], d_depth[1:4, :, half], gen_torch, out=d_out[1:4, :, half])
        assert torch.equal(before, d_color)                        # the image itself is left untouched
        for k in range(1, 4):
            img, m, d = (np.ascontiguousarray(R.eye_of(a[k], eye)) for a in (color, mask, depth))
            percent = orc.decode_depth(d, 1.0)
            assert np.array_equal(sdn.decode_depth_percent(d_depth[k:k + 1, :, half]).cpu().numpy()[0], percent)
            want = E.finish(img, gen_numpy(img[None], m[None], percent[None])[0], m, orc)
            assert np.array_equal(d_out[k, :, half].cpu().numpy(), want), (eye, k)
    assert not d_out[0].any() and not d_out[4].any()
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        sdn.sdiss_infill(d_color[:1, :, :ew], d_mask[:1, :, :ew], d_depth[:1, :, :ew], lambda i, m, d: i.float())
