"""GPU parity of basic_nomal_infill.normal_infill (basic_nomal_infill.py:87-119) through the C ABI: bit-exact against the
oracle's seven plain passes (orc_normal_infill, itself pinned on the reference's function by tests/golden/normal_infill.npz),
on the golden scenes, on random scenes of many shapes, on 1080p frames, on batches and strided side-by-side halves, on the
masks the product default really produces (render -> finish_infill_mask -> normal_infill), and through the file driver."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bni():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import basic_nomal_infill
    return basic_nomal_infill


def ni_scene(rng, W, H, holes=7):
    """An image and a normal-coloured infill mask: discs and rectangles coloured by a direction (some off the border),
    a patch with a zero channel (not `bg` at bni:88 but marching in mark_lower_side), black pixels outside the holes."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(np.stack([xx * 255 // max(W, 1), yy * 255 // max(H, 1), (xx + yy) * 255 // (W + H)], -1)
                  + rng.integers(-40, 41, (H, W, 3)), 1, 255).astype(np.uint8)
    mask = np.zeros((H, W, 3), np.uint8)
    for k in range(holes):
        ang = rng.uniform(0, 2 * np.pi)
        base = np.array([(np.cos(ang) + 1) / 2 * 255, (np.sin(ang) + 1) / 2 * 255, rng.uniform(40, 255)])
        if k % 2:
            x0, y0 = int(rng.integers(-4, max(W - 6, 1))), int(rng.integers(-4, max(H - 6, 1)))
            sel = (xx >= x0) & (xx < x0 + int(rng.integers(2, max(W // 4, 3)))) & (yy >= y0) & (yy < y0 + int(rng.integers(2, max(H // 3, 3))))
        else:
            cx, cy, rad = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, max(H / 4, 3))
            sel = (xx - cx) ** 2 + (yy - cy) ** 2 < rad * rad
        mask[sel] = np.clip(base[None, :] + rng.normal(0, 10, (int(sel.sum()), 3)), 0, 255).astype(np.uint8)
    if H > 12 and W > 16:
        mask[5:9, 10:14] = (200, 0, 90)
        mask[H // 2, W // 3] = (128, 127, 200)
    img[np.all(mask != 0, axis=-1)] = 0
    if H > 8 and W > 12:
        img[H // 2:H // 2 + 3, W // 2:W // 2 + 7] = 0
    return img, mask


def _run(bni, img, mask):
    return bni.normal_infill(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()).cpu().numpy()


def test_golden_scenes(bni, orc, golden):
    g = golden("normal_infill")
    for scene in ("n1", "n2"):
        got = _run(bni, g[f"{scene}_img"], g[f"{scene}_mask"])
        assert np.array_equal(got, orc.normal_infill(g[f"{scene}_img"], g[f"{scene}_mask"])), scene
        assert np.array_equal(got, g[f"{scene}_out"]), scene           # = the reference's normal_infill over restated cv2 calls


@pytest.mark.parametrize("W,H", [(64, 48), (250, 37), (33, 17), (9, 5), (2, 2), (1, 7), (641, 33), (640, 480)])
def test_random_scenes(bni, orc, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    for rep in range(3):
        img, mask = ni_scene(rng, W, H, holes=3 + 4 * rep)
        if rep == 2:
            mask[:] = np.where(mask.any(-1, keepdims=True), mask, 0)
            mask[0, :] = (255, 127, 127); mask[:, 0] = (127, 255, 127)          # holes along two borders: REFLECT_101 and dead rays
            img[0, :] = 0; img[:, 0] = 0
        got = _run(bni, img, mask)
        want, st = orc.normal_infill(img, mask, want_stages=True)
        bad = np.any(got != want, axis=-1)
        assert not bad.any(), f"{W}x{H} rep {rep}: {int(bad.sum())} px differ (bg {int((bad & st['bg']).sum())}, grown {int((bad & st['grown']).sum())})"


def test_full_hd_batch_and_sbs_halves(bni, orc):
    """Four 1080p eyes as two side-by-side frames: strided halves, a batch per half (what process_pair launches)."""
    W, H = 1920, 1080
    rng = np.random.default_rng(77)
    sbs = np.zeros((2, H, 2 * W, 3), np.uint8)
    msk = np.zeros((2, H, 2 * W, 3), np.uint8)
    for f in range(2):
        for e in range(2):
            img, mask = ni_scene(rng, W, H, holes=40)
            sbs[f, :, e * W:(e + 1) * W], msk[f, :, e * W:(e + 1) * W] = img, mask
    got = bni.normal_infill_sbs(torch.from_numpy(sbs).cuda(), torch.from_numpy(msk).cuda()).cpu().numpy()
    for f in range(2):
        for e in range(2):
            sl = slice(e * W, (e + 1) * W)
            want = orc.normal_infill(np.ascontiguousarray(sbs[f, :, sl]), np.ascontiguousarray(msk[f, :, sl]))
            assert np.array_equal(got[f, :, sl], want), (f, e)
    # more images than one launch set holds (16): a batch of 18 small ones
    imgs, masks = zip(*(ni_scene(rng, 96, 64) for _ in range(18)))
    got = bni.normal_infill(torch.from_numpy(np.stack(imgs)).cuda(), torch.from_numpy(np.stack(masks)).cuda()).cpu().numpy()
    for k in range(18):
        assert np.array_equal(got[k], orc.normal_infill(imgs[k], masks[k])), k


def test_product_default_masks(bni, orc):
    """The masks the path really hands over: mesh + --infill_mask + convergence render, finished infill mask, then the
    normal infill of both eyes, every stage against the oracle's."""
    from metric_depth_video_toolbox_amd import stereo_rerender as sr, synthetic
    W, H = 480, 270
    depth_rgb, color = synthetic.SyntheticScene(W, H, seed=5, n_fg=6).frame(0, 100)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
    p = r.frame_params(xfov=45.0, convergence_distance=2.5)
    res = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_seed=True)
    fin = r.finish_infill_mask_sbs(res["seed"])
    out = bni.normal_infill_sbs(res["sbs"], fin).cpu().numpy()
    sbs, fin = res["sbs"].cpu().numpy(), fin.cpu().numpy()
    for e in range(2):
        sl = slice(e * W, (e + 1) * W)
        img, mask = np.ascontiguousarray(sbs[:, sl]), np.ascontiguousarray(fin[:, sl])
        want, st = orc.normal_infill(img, mask, want_stages=True)
        assert st["bg"].sum() > 1000
        assert np.array_equal(out[:, sl], want), e
        holes = np.all(img == 0, -1) & st["bg"]
        assert (out[:, sl][holes].max(-1) > 0).mean() > 0.9          # the holes are filled
    r.close()


def test_argument_checks(bni):
    from metric_depth_video_toolbox_amd import _lib
    img = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.MdvtError):
        bni.normal_infill(img, img.clone(), out=img)                 # d_out may not alias an input
    with pytest.raises(ValueError):
        bni.normal_infill(img, torch.zeros((8, 9, 3), dtype=torch.uint8, device="cuda"))


def test_process_pair_on_frame_dumps(bni, orc, tmp_path):
    W, H, N = 80, 48, 5
    rng = np.random.default_rng(9)
    sbs = np.zeros((N, H, 2 * W, 3), np.uint8); msk = np.zeros((N - 1, H, 2 * W, 3), np.uint8)   # the mask clip ends one frame early
    for f in range(N):
        for e in range(2):
            img, mask = ni_scene(rng, W, H)
            sbs[f, :, e * W:(e + 1) * W] = img
            if f < N - 1:
                msk[f, :, e * W:(e + 1) * W] = mask
    cpath, mpath = str(tmp_path / "clip_stereo.npy"), str(tmp_path / "clip_stereo.npy_infillmask.npy")
    np.save(cpath, sbs); np.save(mpath, msk)
    final = bni.process_pair(cpath, mpath, batch=2)
    assert final == str(tmp_path / "clip_stereo.npy_infilled.npy") and not os.path.exists(str(tmp_path / "clip_stereo.npy_tmp_infilled.npy"))
    got = np.load(final)
    assert got.shape == sbs.shape
    for f in range(N):
        for e in range(2):
            sl = slice(e * W, (e + 1) * W)
            m = msk[f, :, sl] if f < N - 1 else np.zeros((H, W, 3), np.uint8)
            assert np.array_equal(got[f, :, sl], orc.normal_infill(np.ascontiguousarray(sbs[f, :, sl]), np.ascontiguousarray(m))), (f, e)
    assert np.array_equal(got[N - 1], sbs[N - 1])                     # no mask: nothing changes
    assert np.load(bni.process_pair(cpath, mpath, max_frames=2)).shape[0] == 2


def test_batched_basic_infill_is_the_per_eye_loop(bni, orc):
    """mdvt_infill_using_mask_normals (sr:809-812 for a batch, normals read from the u8 mask, filled in place) against the
    oracle's infill_using_normals fed with NumPy's ((mask / 255) * 2 - 1) in f32 -- on strided side-by-side halves."""
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    rng = np.random.default_rng(31)
    for W, H, N in ((96, 64, 3), (250, 37, 2), (33, 17, 1), (640, 360, 2)):
        sbs = np.zeros((N, H, 2 * W, 3), np.uint8); msk = np.zeros_like(sbs); hole = np.zeros((N, H, 2 * W), np.uint8)
        for f in range(N):
            for e in range(2):
                img, mask = ni_scene(rng, W, H)
                h = np.any(mask != 0, -1)                                   # the hole plane of the render: mask != black <=> hole
                img[h] = 0
                sbs[f, :, e * W:(e + 1) * W], msk[f, :, e * W:(e + 1) * W], hole[f, :, e * W:(e + 1) * W] = img, mask, h * 255
        d_sbs, d_msk, d_hole = torch.from_numpy(sbs).cuda(), torch.from_numpy(msk).cuda(), torch.from_numpy(hole).cuda()
        for e in range(2):
            sl = slice(e * W, (e + 1) * W)
            sr.infill_using_mask_normals(d_sbs[:, :, sl], d_hole[:, :, sl], d_msk[:, :, sl], out=d_sbs[:, :, sl])     # in place
        got = d_sbs.cpu().numpy()
        for f in range(N):
            for e in range(2):
                sl = slice(e * W, (e + 1) * W)
                wn = ((msk[f, :, sl].astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)              # sr:808, 810
                want = orc.infill_using_normals(np.ascontiguousarray(sbs[f, :, sl]), hole[f, :, sl] > 0, wn)
                assert np.array_equal(got[f, :, sl], want), (W, H, f, e)
        # a copy instead of in place, and fewer steps
        out = sr.infill_using_mask_normals(torch.from_numpy(sbs[0, :, :W].copy()).cuda(), torch.from_numpy(hole[0, :, :W].copy()).cuda() > 0,
                                           torch.from_numpy(msk[0, :, :W].copy()).cuda(), max_steps=5).cpu().numpy()
        wn = ((msk[0, :, :W].astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)
        assert np.array_equal(out, orc.infill_using_normals(np.ascontiguousarray(sbs[0, :, :W]), hole[0, :, :W] > 0, wn, 5))


def test_torch_division_by_255_is_the_reference_division():
    """The reference's normals are `u8.astype(float32) / 255.0` in NumPy (sr:808): a correctly rounded f32 division.  Torch on
    the device may multiply by a reciprocal instead; the batched kernel divides.  All 256 inputs."""
    v = torch.arange(256, dtype=torch.uint8, device="cuda")
    t = ((v.to(torch.float32) / 255.0) * 2 - 1).cpu().numpy()
    n = ((np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)
    diff = int((t.view(np.uint32) != n.view(np.uint32)).sum())
    print(f"torch (x / 255.0) * 2 - 1 differs from NumPy's on {diff} of 256 inputs")
    # (informational: the clip driver no longer computes normals with torch)


def test_more_images_than_a_launch_set_and_argument_checks_of_the_batched_infill(bni, orc):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr, _lib
    rng = np.random.default_rng(41)
    W, H, N = 80, 48, 19                                                       # 19 > 16 images per launch set
    imgs, masks = zip(*(ni_scene(rng, W, H) for _ in range(N)))
    imgs, masks = np.stack(imgs), np.stack(masks)
    hole = np.any(masks != 0, -1)
    imgs[hole] = 0
    got = sr.infill_using_mask_normals(torch.from_numpy(imgs).cuda(), torch.from_numpy(hole).cuda(), torch.from_numpy(masks).cuda()).cpu().numpy()
    for k in range(N):
        wn = ((masks[k].astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)
        assert np.array_equal(got[k], orc.infill_using_normals(imgs[k], hole[k], wn)), k
    img = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.MdvtError):
        sr.infill_using_mask_normals(img, torch.zeros((8, 8), dtype=torch.uint8, device="cuda"), img, out=img)     # d_img may not alias the mask image
    with pytest.raises(ValueError):
        sr.infill_using_mask_normals(img, torch.zeros((8, 9), dtype=torch.uint8, device="cuda"), img.clone())


def test_ultra_hd_frame(bni, orc):
    """3840 x 2160 (BASELINE config 4's size): 30 x 135 tiles, sub-list capacities, 32-bit offsets."""
    W, H = 3840, 2160
    rng = np.random.default_rng(2160)
    img, mask = ni_scene(rng, W, H, holes=60)
    got = _run(bni, img, mask)
    want, st = orc.normal_infill(img, mask, want_stages=True)
    assert st["bg"].sum() > 100000 and st["grown"].sum() > 10000
    assert np.array_equal(got, want)


def test_cli_batch_mode_keeps_going_after_a_failed_clip(bni, orc, tmp_path, capsys):
    """basic_nomal_infill.py:246-276: .txt lists of clips; a clip that fails is reported, the others are processed."""
    W, H = 64, 40
    rng = np.random.default_rng(12)
    paths = []
    for k in range(2):
        sbs = np.zeros((2, H, 2 * W, 3), np.uint8); msk = np.zeros_like(sbs)
        for f in range(2):
            for e in range(2):
                sbs[f, :, e * W:(e + 1) * W], msk[f, :, e * W:(e + 1) * W] = ni_scene(rng, W, H)
        c, m = str(tmp_path / f"clip{k}_stereo.npy"), str(tmp_path / f"clip{k}_stereo.npy_infillmask.npy")
        np.save(c, sbs); np.save(m, msk)
        paths.append((c, m, sbs, msk))
    (tmp_path / "colors.txt").write_text(f"{paths[0][0]}\n{tmp_path / 'nope.npy'}\n# comment\n{paths[1][0]}\n")
    (tmp_path / "masks.txt").write_text(f"{paths[0][1]}\n{tmp_path / 'nope_mask.npy'}\n{paths[1][1]}\n")
    assert bni.main(["--sbs_color_video", str(tmp_path / "colors.txt"), "--sbs_mask_video", str(tmp_path / "masks.txt")]) == 0
    out = capsys.readouterr().out
    assert "Batch mode: 3 pairs" in out and "[ERROR] A clip failed" in out and out.count("Done. Wrote:") == 2
    for c, m, sbs, msk in paths:
        got = np.load(c + "_infilled.npy")
        for f in range(2):
            for e in range(2):
                sl = slice(e * W, (e + 1) * W)
                assert np.array_equal(got[f, :, sl], orc.normal_infill(np.ascontiguousarray(sbs[f, :, sl]), np.ascontiguousarray(msk[f, :, sl])))
