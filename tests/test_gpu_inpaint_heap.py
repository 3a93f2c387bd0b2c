"""GPU tests of the infill-mask completion in cv2.inpaint's heap order (mdvt_finish_infill_mask_heap[_stereo],
StereoRerenderer.finish_infill_mask(order="heap"), --inpaint_order heap).  The reference is the oracle's sequential heap march
(orc.telea_fmm on the mask key-coloured OR black, radius 3), the sr:807 merge and orc.masked_blur; every comparison is exact."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GREEN = (0, 255, 0)
FAILED = -1                     # 0xFFFFFFFF in the int32 remaining tensor: a loop bound tripped


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import stereo_rerender, synthetic
    return stereo_rerender, synthetic


def fmm_finish(orc, seed, key=GREEN):
    """sr:803-808 with cv2.inpaint's own order -> (finished image, key-coloured pixels the march never reaches)."""
    keym = np.all(seed == np.array(key, np.uint8), -1)
    mask = (keym | np.all(seed == 0, -1)).astype(np.uint8)
    filled = orc.telea_fmm(seed, mask)
    merged = seed.copy()
    merged[keym] = filled[keym]
    return orc.masked_blur(merged)


def unreachable_keys(seed, key=GREEN):
    """Key-coloured pixels in 4-connected components of the mask that hold no known pixel's neighbour."""
    from scipy import ndimage
    keym = np.all(seed == np.array(key, np.uint8), -1)
    mask = keym | np.all(seed == 0, -1)
    lab, n = ndimage.label(mask)
    known_nb = ndimage.binary_dilation(~mask, structure=ndimage.generate_binary_structure(2, 1)) & mask
    reached = np.unique(lab[known_nb])
    return int((keym & ~np.isin(lab, reached)).sum())


def _synthetic_seed(rng, W, H, key=GREEN):
    seed = np.zeros((H, W, 3), np.uint8)
    for _ in range(5):                                      # holes: key colour, normal-coloured points along their edges
        x0, y0 = int(rng.integers(1, W - 12)), int(rng.integers(1, H - 12))
        w, h = int(rng.integers(4, max(5, W // 4))), int(rng.integers(4, max(5, H // 3)))
        seed[y0:y0 + h, x0:x0 + w] = key
        for _ in range(w + h):
            seed[min(H - 1, y0 + int(rng.integers(0, h))), min(W - 1, x0 + int(rng.integers(0, 2)))] = rng.integers(1, 255, 3)
            seed[min(H - 1, y0 + h), min(W - 1, x0 + int(rng.integers(0, w)))] = rng.integers(1, 255, 3)
    return seed


def _check(got, rem, wants, rems):
    for k, (w, wr) in enumerate(zip(wants, rems)):
        assert np.array_equal(got[k], w), k
        assert int(rem[k]) == wr, k


@pytest.mark.parametrize("W,H", [(96, 64), (250, 61)])
def test_heap_order_matches_the_sequential_march(mods, orc, W, H):
    sr, _ = mods
    rng = np.random.default_rng(7 * W + H)
    seeds = np.stack([_synthetic_seed(rng, W, H) for _ in range(4)])
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    got, rem = r.finish_infill_mask(torch.from_numpy(seeds).cuda(), want_remaining=True, order="heap")
    _check(got.cpu().numpy(), rem.cpu().numpy(), [fmm_finish(orc, s) for s in seeds], [unreachable_keys(s) for s in seeds])
    one = r.finish_infill_mask(torch.from_numpy(seeds[1]).cuda(), order="heap")                   # a single [H, W, 3] image
    assert np.array_equal(one.cpu().numpy(), fmm_finish(orc, seeds[1]))
    r.close()


def test_ties_straight_rims_and_a_single_known_pixel(mods, orc):
    sr, _ = mods
    W, H = 120, 80
    rims = np.zeros((H, W, 3), np.uint8)
    rims[:] = GREEN
    rims[0, :] = (200, 40, 90)                                  # a straight rim along the top: T ties along the whole row
    rims[:, 0] = (30, 180, 70)                                  # and down the left side
    rims[H - 1, W // 2:] = (90, 90, 250)
    rims[40:, 60] = 0                                           # a black wall: filled, but not kept
    single = np.zeros((H, W, 3), np.uint8)
    single[:] = GREEN
    single[H // 2, W // 3] = (120, 60, 210)                     # one known pixel in a large hole
    seeds = np.stack([rims, single])
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    got, rem = r.finish_infill_mask(torch.from_numpy(seeds).cuda(), want_remaining=True, order="heap")
    _check(got.cpu().numpy(), rem.cpu().numpy(), [fmm_finish(orc, s) for s in seeds], [0, 0])
    r.close()


def test_random_half_mask_with_a_black_key(mods, orc):
    """Window 0 holds every known pixel next to the mask (~10^5 pops: the sort that does not fit LDS); the mask touches all four
    borders.  Black key: every black pixel is filled and kept."""
    sr, _ = mods
    W, H = 640, 480
    rng = np.random.default_rng(5)
    seed = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
    hole = rng.random((H, W)) < 0.5
    hole[0, :] = hole[-1, :] = True
    hole[:, 0] = hole[:, -1] = True
    seed[hole] = 0
    r = sr.StereoRerenderer(W, H)
    assert tuple(r.key_rgb) == (0, 0, 0)
    got, rem = r.finish_infill_mask(torch.from_numpy(seed).cuda(), want_remaining=True, order="heap")
    assert int(rem[0]) == 0
    assert np.array_equal(got.cpu().numpy(), fmm_finish(orc, seed, key=(0, 0, 0)))
    r.close()


def test_degenerate_images(mods, orc):
    sr, _ = mods
    W, H = 64, 48
    rng = np.random.default_rng(11)
    nothing = rng.integers(1, 200, (H, W, 3), dtype=np.uint8)                 # no pixel to fill
    nothing[..., 1] = np.minimum(nothing[..., 1], 200)                        # (never the key colour)
    unknown = np.zeros((H, W, 3), np.uint8)                                   # no known pixel at all
    unknown[10:30, 5:50] = GREEN
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    got, rem = r.finish_infill_mask(torch.from_numpy(np.stack([nothing, unknown])).cuda(), want_remaining=True, order="heap")
    got, rem = got.cpu().numpy(), rem.cpu().numpy()
    assert np.array_equal(got[0], orc.masked_blur(nothing)) and int(rem[0]) == 0
    assert int(rem[1]) == 20 * 45
    assert np.array_equal(got[1], orc.masked_blur(unknown)) and np.array_equal(got[1], fmm_finish(orc, unknown))
    r.close()


def test_wide_and_tall_image(mods, orc):
    sr, _ = mods
    W, H = 2112, 1100
    rng = np.random.default_rng(3)
    seed = _synthetic_seed(rng, W, H)
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    got, rem = r.finish_infill_mask(torch.from_numpy(seed).cuda(), want_remaining=True, order="heap")
    assert int(rem[0]) == unreachable_keys(seed)
    assert np.array_equal(got.cpu().numpy(), fmm_finish(orc, seed))
    r.close()


def test_side_by_side_strided_views(mods, orc):
    sr, _ = mods
    W, H, N = 96, 64, 10
    rng = np.random.default_rng(17)
    pool = [_synthetic_seed(rng, W, H) for _ in range(5)]
    sbs = np.stack([np.concatenate([pool[f % 5], pool[(f * 3 + 1) % 5]], 1) for f in range(N)])
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    got, rem = r.finish_infill_mask_sbs(torch.from_numpy(sbs).cuda(), want_remaining=True, order="heap")
    got, rem = got.cpu().numpy(), rem.cpu().numpy()
    assert rem.shape == (2, N)
    fins = [fmm_finish(orc, s) for s in pool]
    unr = [unreachable_keys(s) for s in pool]
    for f in range(N):
        assert np.array_equal(got[f][:, :W], fins[f % 5]), f
        assert np.array_equal(got[f][:, W:], fins[(f * 3 + 1) % 5]), f
        assert rem[0, f] == unr[f % 5] and rem[1, f] == unr[(f * 3 + 1) % 5]
    r.close()


@pytest.mark.parametrize("conv", [2.5, None])
def test_product_default_seeds_at_1080p(mods, orc, conv):
    """Seeds of a real render (mesh, --infill_mask, with and without 2.5 m convergence), both eyes: the heap order gives the
    sequential march's bytes, and differs from the level order in key-coloured pixels."""
    sr, synthetic = mods
    W, H = 1920, 1080
    d, c = synthetic.SyntheticScene(W, H, config_id=2).frame(0)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
    p = r.frame_params(xfov=45.0, convergence_distance=conv) if conv else r.frame_params(xfov=45.0)
    seed = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_seed=True)["seed"]
    heap, rem = r.finish_infill_mask_sbs(seed, want_remaining=True, order="heap")
    levels = r.finish_infill_mask_sbs(seed)
    seed, heap, levels = seed.cpu().numpy(), heap.cpu().numpy(), levels.cpu().numpy()
    assert rem.shape == (2, 1) and not (rem == FAILED).any()
    for e, sl in enumerate((slice(0, W), slice(W, 2 * W))):
        s = np.ascontiguousarray(seed[:, sl])
        keym = np.all(s == GREEN, -1)
        assert keym.sum() > 1000
        assert int(rem[e, 0]) == unreachable_keys(s)
        assert np.array_equal(heap[:, sl], fmm_finish(orc, s)), e
        assert (heap[:, sl][keym] != levels[:, sl][keym]).any(-1).sum() > 0
    r.close()


def test_batch_independence(mods, orc):
    sr, _ = mods
    W, H = 96, 64
    rng = np.random.default_rng(23)
    seeds = np.stack([_synthetic_seed(rng, W, H) for _ in range(64)])
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    alone = r.finish_infill_mask(torch.from_numpy(seeds[37]).cuda(), order="heap").cpu().numpy()
    t = torch.from_numpy(seeds).cuda()
    a, ra = r.finish_infill_mask(t, want_remaining=True, order="heap")
    b, rb = r.finish_infill_mask(t, want_remaining=True, order="heap")
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a[37], alone) and np.array_equal(a, b)
    assert torch.equal(ra, rb) and not (ra == FAILED).any()
    assert np.array_equal(alone, fmm_finish(orc, seeds[37]))
    r.close()


def test_order_arguments_are_checked(mods):
    sr, _ = mods
    r = sr.StereoRerenderer(32, 24, infill_mask=True)
    seed = torch.zeros((24, 32, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        r.finish_infill_mask(seed, max_rounds=5, order="heap")
    with pytest.raises(ValueError):
        r.finish_infill_mask(seed, order="fifo")
    sbs = torch.zeros((1, 24, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        r.finish_infill_mask_sbs(sbs, no_host_wait=True, order="heap")
    with pytest.raises(ValueError):
        r.finish_infill_mask_sbs(sbs, max_rounds=-3, order="heap")
    r.close()


def test_cli_with_the_heap_order(mods, orc, tmp_path, capsys):
    """--infill_mask --inpaint_order heap through files: the _infillmask frames are the sequential march's composition of the
    oracle's own seed images."""
    sr, synthetic = mods
    W, H, N = 160, 90, 5
    d, c = synthetic.SyntheticScene(W, H, config_id=3, n_fg=5).clip(N)
    dp, cp = str(tmp_path / "v_depth.npy"), str(tmp_path / "v.npy")
    np.save(dp, d); np.save(cp, c)
    rc = sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "50", "--pupillary_distance", "65",
                  "--infill_mask", "--inpaint_order", "heap", "--batch", "3"])
    assert rc == 0 and "Processing complete" in capsys.readouterr().out
    finished = np.load(dp + "_stereo.npy_infillmask.npy")
    assert finished.shape == (N, H, 2 * W, 3)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
    p = r.frame_params(xfov=50.0)
    K = np.array([p.K[k] for k in range(9)]).reshape(3, 3)
    op = orc.make_params(W, H, K, ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale, mode=orc.MODE_MESH,
                         remove_edges=True, edge_points=True, key_rgb=GREEN)
    for t in range(N):
        want = orc.render_stereo(op, d[t], c[t], want_seed=True)
        assert np.array_equal(finished[t][:, :W], fmm_finish(orc, want["left_seed"])), t
        assert np.array_equal(finished[t][:, W:], fmm_finish(orc, want["right_seed"])), t
    r.close()
