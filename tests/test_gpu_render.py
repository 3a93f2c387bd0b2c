"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs, and against the committed golden fixtures.  Bar: bit-exact hole mask, RGB and depth planes
(the <= 1 LSB RGB allowance of the north star is not needed: both sides follow one arithmetic decree).

Exact depth ties between overlapping triangles go to the triangle drawn first (GL_LESS + the draw order of
dmt:1243-1254) on both sides; test_exact_depth_ties_follow_the_draw_order builds scenes that are full of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, synthetic
    return _lib, stereo_rerender, synthetic


def _K(p):
    return np.array([p.K[k] for k in range(9)]).reshape(3, 3)


def _oracle(orc, r, p, depth_rgb, color, T=None, want_depth=True):
    op = orc.make_params(r.W, r.H, _K(p), ipd_m=r.pupillary_distance / 1000, max_depth=r.max_depth,
                         depth_scale=p.depth_scale,
                         mode=orc.MODE_POINTS if r.mode == 0 else orc.MODE_MESH,
                         remove_edges=r.remove_edges, edge_points=r.edge_points,
                         conv_angle=p.convergence_angle, T=T, key_rgb=r.key_rgb, cull=getattr(r, "cull", 0),
                         subpixel_bits=getattr(r, "subpixel_bits", 0))
    return orc.render_stereo(op, depth_rgb, color, want_depth=want_depth)


def _compare(got, want, W, tag=""):
    sbs, mask = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy()
    for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
        m, wm = mask[:, sl], want[eye + "_mask"]
        assert np.array_equal(m, wm), f"{tag} {eye} mask differs at {int((m != wm).sum())} px"
        c, wc = sbs[:, sl], want[eye + "_rgb"]
        assert np.array_equal(c, wc), f"{tag} {eye} rgb differs at {int(np.any(c != wc, axis=-1).sum())} px"
        if "depth" in got:
            z, wz = got["depth"].cpu().numpy()[:, sl], want[eye + "_depth"]
            assert np.array_equal(z.view(np.uint32), wz.view(np.uint32)), f"{tag} {eye} depth plane differs"


def _scene(synthetic, W, H, seed, n_fg=6, max_depth=100, zero_patch=True, key_px=True):
    depth_rgb, color = synthetic.SyntheticScene(W, H, seed=seed, n_fg=n_fg).frame(0, max_depth)
    if zero_patch and H > 8 and W > 16:
        depth_rgb[3:6, 5:11] = 0                # Z = 0: rejected by the near plane
        depth_rgb[H - 2, W - 3] = (0, 0, 1)     # one depth LSB: 1.55 mm
    if key_px and H > 8 and W > 16:
        color[1, 2] = (0, 0, 0)                 # exact key colours inside the image: colour-key rule
        color[2, 7] = (0, 255, 0)
        color[H // 2, W // 2] = (0, 0, 0)
    return depth_rgb, color


SIZES = [(64, 48), (96, 64), (250, 37), (33, 17), (640, 480)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("infill_mask", [False, True])
def test_points_pure_shift(mods, orc, W, H, infill_mask):
    _lib, sr, synthetic = mods
    depth_rgb, color = _scene(synthetic, W, H, seed=W * 1000 + H)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True,
                            infill_mask=infill_mask, dont_remove_edges=True)
    p = r.frame_params(xfov=45.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"points {W}x{H}")
    assert (got["mask"] > 0).any() and not (got["mask"] > 0).all()
    r.close()


@pytest.mark.parametrize("xfov,master,max_depth,ipd", [(60.0, 45.0, 100, 63), (35.0, 45.0, 20, 70), (45.0, 70.0, 655, 65)])
def test_points_scaled_depth_and_other_scalars(mods, orc, xfov, master, max_depth, ipd):
    _lib, sr, synthetic = mods
    W, H = 128, 72
    depth_rgb, color = _scene(synthetic, W, H, seed=77, max_depth=max_depth)
    r = sr.StereoRerenderer(W, H, pupillary_distance=ipd, max_depth=max_depth, master_xfov=master, render_as_pointcloud=True)
    p = r.frame_params(xfov=xfov)
    assert p.depth_scale != 1.0
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, "scaled")
    r.close()


def test_points_without_depth_planes_and_sbs_layout(mods, orc):
    _lib, sr, synthetic = mods
    W, H = 192, 108
    depth_rgb, color = _scene(synthetic, W, H, seed=5)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p)
    assert "depth" not in got and tuple(got["sbs"].shape) == (H, 2 * W, 3) and tuple(got["mask"].shape) == (H, 2 * W)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, "no-depth")
    r.close()


@pytest.mark.parametrize("case", ["convergence", "pose", "both"])
@pytest.mark.parametrize("W,H", [(96, 64), (250, 37)])
def test_points_general_path(mods, orc, case, W, H):
    _lib, sr, synthetic = mods
    depth_rgb, color = _scene(synthetic, W, H, seed=31)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    T = None
    if case in ("pose", "both"):
        T = synthetic.synthetic_pose_track(40)[37]
    p = r.frame_params(xfov=45.0, convergence_distance=2.5 if case != "pose" else None, transformation=T)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color, T=T), W, f"general/{case}")
    r.close()


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("edge_points", [False, True])
def test_points_remove_edges(mods, orc, general, edge_points):
    _lib, sr, synthetic = mods
    W, H = 160, 96
    depth_rgb, color = _scene(synthetic, W, H, seed=9)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True, infill_mask=True,
                            dont_place_points_in_edges=not edge_points)
    assert r.remove_edges and r.edge_points == edge_points and r.key_rgb == (0, 255, 0)
    p = r.frame_params(xfov=45.0, convergence_distance=3.0 if general else None)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"remove_edges general={general} edge={edge_points}")
    r.close()


def test_batch_with_per_frame_parameters(mods, orc):
    _lib, sr, synthetic = mods
    W, H, N = 128, 80, 11
    sc = synthetic.SyntheticScene(W, H, seed=3, n_fg=5)
    d, c = sc.clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    params = [r.frame_params(xfov=40.0 + k) for k in range(N)]           # xfov file: one FOV per frame (sr:515-518)
    got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), params, want_depth=True)
    for k in range(N):
        one = {key: v[k] for key, v in got.items()}
        _compare(one, _oracle(orc, r, params[k], d[k], c[k]), W, f"batch frame {k}")
    r.close()


def test_full_hd_single_frame_matches_oracle(mods, orc):
    """BASELINE config C2: 1920x1080, 65 mm baseline, bit-exact hole mask vs the CPU restatement."""
    _lib, sr, synthetic = mods
    W, H = 1920, 1080
    depth_rgb, color = synthetic.SyntheticScene(W, H, config_id=2).frame(0)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, "C2")
    r.close()


# ----------------------------------------------------------------------------------------------- mesh mode
@pytest.mark.parametrize("W,H", [(64, 48), (96, 64), (250, 37), (33, 17), (320, 240), (640, 480)])
@pytest.mark.parametrize("infill_mask", [False, True])
def test_mesh_pure_shift(mods, orc, W, H, infill_mask):
    """Default mode of the reference (grid mesh).  infill_mask=True is the product default of
    movie_2_3D.py: 89-degree edge filter + green key + edge points (m23d:441, sr:568-570)."""
    _lib, sr, synthetic = mods
    depth_rgb, color = _scene(synthetic, W, H, seed=W * 7 + H)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=infill_mask)
    p = r.frame_params(xfov=45.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"mesh {W}x{H} infill={infill_mask}")
    assert (got["mask"] > 0).any() and not (got["mask"] > 0).all()
    r.close()


@pytest.mark.parametrize("flags", [dict(remove_edges=True, dont_place_points_in_edges=True), dict(remove_edges=True)])
def test_mesh_remove_edges_variants(mods, orc, flags):
    _lib, sr, synthetic = mods
    W, H = 160, 96
    depth_rgb, color = _scene(synthetic, W, H, seed=21)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, **flags)
    p = r.frame_params(xfov=60.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"mesh {flags}")
    r.close()


@pytest.mark.parametrize("case", ["convergence", "pose", "both"])
@pytest.mark.parametrize("infill_mask", [False, True])
def test_mesh_general_path(mods, orc, case, infill_mask):
    _lib, sr, synthetic = mods
    W, H = 96, 64
    depth_rgb, color = _scene(synthetic, W, H, seed=41)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=infill_mask)
    T = synthetic.synthetic_pose_track(40)[33] if case in ("pose", "both") else None
    p = r.frame_params(xfov=45.0, convergence_distance=2.5 if case != "pose" else None, transformation=T)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color, T=T), W, f"mesh general/{case}")
    r.close()


@pytest.mark.parametrize("W,H", [(64, 48), (96, 64), (256, 144), (320, 240), (8, 2), (36, 300), (1000, 40)])
@pytest.mark.parametrize("flags", [dict(), dict(infill_mask=True), dict(remove_edges=True, dont_place_points_in_edges=True)])
def test_mesh_convergence_only_band_kernel(mods, orc, W, H, flags, monkeypatch):
    """Mesh + per-frame convergence and nothing else (movie_2_3D.py:433-445): k_mesh_conv keeps the scanline's z-buffer in LDS
    instead of the global-key kernels' round trips.  Several toe-in angles in one batch (incl. one too strong for the kernel,
    which the host sends down the general path), depth planes and seed images; then the same batch without MDVT_MESH_CONV=1
    (general path for every frame) must give the same bytes."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")          # the hooks below exist in the tuning build only (csrc/mdvt_internal.h)
    _lib, sr, synthetic = mods
    monkeypatch.setenv("MDVT_MESH_CONV", "1")                # the kernel is opt-in (it does not beat the general path: profiles/r03_conv_band.md)
    convs = [2.5, 8.0, 1.2, 0.9, 0.25]
    frames = [_scene(synthetic, W, H, seed=500 + 13 * k + W, n_fg=3 + k % 3) for k in range(len(convs))]
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, **flags)
    ps = [r.frame_params(xfov=45.0 + 5 * (k % 2), convergence_distance=cd) for k, cd in enumerate(convs)]
    d = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    c = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    seed = bool(flags.get("infill_mask"))
    got = r.render(d, c, ps, want_depth=True, want_seed=seed)
    for k in range(len(convs)):
        op = orc.make_params(W, H, _K(ps[k]), ipd_m=0.065, max_depth=100, depth_scale=ps[k].depth_scale, mode=orc.MODE_MESH,
                             remove_edges=r.remove_edges, edge_points=int(r.edge_points), conv_angle=ps[k].convergence_angle, key_rgb=r.key_rgb)
        want = orc.render_stereo(op, frames[k][0], frames[k][1], want_depth=True, want_seed=seed)
        _compare({key: got[key][k] for key in ("sbs", "mask", "depth")}, want, W, f"conv band {W}x{H} {flags} conv={convs[k]}")
        if seed:
            for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                assert np.array_equal(got["seed"][k][:, sl].cpu().numpy(), want[eye + "_seed"]), f"conv band seed {eye} conv={convs[k]}"
    monkeypatch.delenv("MDVT_MESH_CONV")
    ref = r.render(d, c, ps, want_depth=True, want_seed=seed)           # the general path, its rasteriser = k_mesh_raster_conv (default)
    monkeypatch.setenv("MDVT_RASTER_CONV_OFF", "1")
    ref2 = r.render(d, c, ps, want_depth=True, want_seed=seed)          # ... = k_mesh_raster_small (what poses take)
    for key in got:
        assert torch.equal(got[key], ref[key]), f"k_mesh_conv and the general path disagree on {key}"
        assert torch.equal(got[key], ref2[key]), f"the two rasterisers of the general path disagree on {key}"
    r.close()


@pytest.mark.parametrize("kernel", ["k_mesh_conv", "k_mesh_raster_conv"])
def test_mesh_convergence_band_kernel_on_hard_scenes(mods, orc, monkeypatch, kernel):
    """The two convergence-only kernels (k_mesh_conv: opt-in, z-buffer in LDS; k_mesh_raster_conv: the general path's default
    rasteriser for such frames) on what stresses their special cases: the contention band of C4 (hundreds of cells folded onto a few
    pixels: exact depth ties, stretched cells, twisted cells), alternating near / far columns, sub-millimetre and zero depths
    (near plane), face culling, a toe-in just inside the kernel's admission bound, and forced tie passes."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")          # the hooks below exist in the tuning build only (csrc/mdvt_internal.h)
    from metric_depth_video_toolbox_amd.depth_map_tools import compute_camera_matrix
    _lib, sr, synthetic = mods
    if kernel == "k_mesh_conv":
        monkeypatch.setenv("MDVT_MESH_CONV", "1")
    rng = np.random.default_rng(77)
    cases = []
    for (W, H, t) in ((256, 96, 180), (256, 64, 299)):
        K = compute_camera_matrix(45.0, None, W, H)
        sc = synthetic.SyntheticScene(W, H, config_id=4)
        z = synthetic.contention_band(sc.depth_m(t), K[0, 0], 0.065, row0=H // 3, rows=H // 3)
        cases.append((synthetic.quantise_depth_to_rgb(z), sc.frame(t)[1]))
    W, H = 256, 96
    for style in range(4):
        d = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if style == 0:      # alternating near / far columns
            code = np.where((np.arange(W)[None, :] // 2) % 2 == 0, 150, 30000).astype(np.uint32) + np.zeros((H, 1), np.uint32)
        elif style == 1:    # very near content: codes 0..3 (Z = 0 rejected by the near plane)
            code = rng.integers(0, 4, (H, W)).astype(np.uint32)
        elif style == 2:    # one-code noise on a slope
            code = (3000 + np.arange(W)[None, :] // 3 + rng.integers(0, 2, (H, W))).astype(np.uint32)
        else:               # rectangles over a far plane
            code = np.full((H, W), 40000, np.uint32); code[20:60, 40:90] = 500; code[5:90, 150:160] = 90; code[70:, :] = 2500
        d[..., 0] = (code >> 8) & 0xFF; d[..., 2] = code & 0xFF
        cases.append((d, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)))
    for n, (depth_rgb, color) in enumerate(cases):
        H, W = depth_rgb.shape[:2]
        for kw, conv in ((dict(), 2.5), (dict(infill_mask=True), 1.5), (dict(cull=1), 2.0), (dict(cull=2, remove_edges=True), 3.0), (dict(), 0.62)):
            r = sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)
            p = r.frame_params(xfov=45.0, convergence_distance=conv)
            want = _oracle(orc, r, p, depth_rgb, color)
            for dbg in (None, "32"):
                if dbg:
                    monkeypatch.setenv("MDVT_DEBUG_SKIP", dbg)
                got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
                _compare(got, want, W, f"conv band hard scene {n} {kw} conv={conv} dbg={dbg}")
                monkeypatch.delenv("MDVT_DEBUG_SKIP", raising=False)
            r.close()


@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_general_paths_reuse_their_key_planes_across_submissions(mods, orc, mode):
    """The z-key planes of the general paths are never cleared between submissions: a slot's uses alternate in parity
    (atomicMin / atomicMax), the resolve rewrites only the words a use left uncovered, the edge-key words are emptied from a
    list.  One renderer, a sequence of submissions of different batch sizes, scenes, poses and hole patterns -- every slot
    sees both parities, slots see different numbers of uses -- each compared bit for bit with the oracle."""
    _lib, sr, synthetic = mods
    W, H = 96, 64
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True, render_as_pointcloud=(mode == "points"))
    track = synthetic.synthetic_pose_track(40)
    step = 0
    for n, conv in ((3, 2.5), (1, 1.2), (5, None), (2, 4.0), (5, 2.0), (1, None), (4, 0.8)):
        frames = [_scene(synthetic, W, H, seed=300 + 7 * step + k, n_fg=2 + (step + k) % 4) for k in range(n)]
        Ts = [track[(5 * step + 3 * k) % 40] if (conv is None or k % 2) else None for k in range(n)]
        ps = [r.frame_params(xfov=45.0, convergence_distance=conv, transformation=Ts[k]) for k in range(n)]
        d = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
        c = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
        got = r.render(d, c, ps, want_depth=True)
        for k in range(n):
            one = {key: (v[k] if hasattr(v, "shape") and v.dim() > 0 and v.shape[0] == n else v) for key, v in got.items()}
            _compare(one, _oracle(orc, r, ps[k], frames[k][0], frames[k][1], T=Ts[k]), W, f"{mode} submission {step} frame {k}")
        step += 1
    r.close()


@pytest.mark.parametrize("cull", [1, 2])
@pytest.mark.parametrize("variant", ["band", "rows_odd_width", "rows_edges", "general", "general_edges", "wide_global"])
def test_mesh_face_culling(mods, orc, cull, variant, monkeypatch):
    """mdvt_config.cull: Open3D's legacy mesh_show_back_face defaults to off and dmt:1507-1556 never sets it; whether that
    means GL_CULL_FACE cannot be observed here, so both candidates exist.  The grid's own winding is the front face:
    culling back faces removes the fold-over triangles of the rubber sheet, culling front faces leaves only those."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")          # the hooks below exist in the tuning build only (csrc/mdvt_internal.h)
    _lib, sr, synthetic = mods
    W, H = (250, 61) if variant == "rows_odd_width" else (256, 64)
    depth_rgb, color = _scene(synthetic, W, H, seed=90 + cull)
    if variant == "wide_global":
        monkeypatch.setenv("MDVT_FORCE_GLOBAL", "1")
    kw = dict(infill_mask=True) if variant in ("rows_edges", "general_edges") else {}
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, cull=cull, **kw)
    T = synthetic.synthetic_pose_track(40)[21] if variant.startswith("general") else None
    p = r.frame_params(xfov=45.0, convergence_distance=2.0 if variant.startswith("general") else None, transformation=T)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    want = _oracle(orc, r, p, depth_rgb, color, T=T)
    _compare(got, want, W, f"cull={cull} {variant}")
    both = sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)
    ref = both.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p)
    if cull == 2:        # only the fold-over triangles are left: almost everything becomes a hole
        assert float((got["mask"] > 0).float().mean()) > 0.8
    else:                # back faces lie behind the surface that folds over them: removing them uncovers nothing ...
        assert bool(((got["mask"] > 0) | (ref["mask"] == 0)).all())
    r.close(); both.close()


def test_exact_depth_ties_follow_the_draw_order(mods, orc, monkeypatch):
    """GL_LESS keeps the triangle drawn first on an exact depth tie (draw order: all tri1 row-major, then all tri2,
    dmt:1243-1254).  C4's contention band (hundreds of cells folded onto a few pixels) produces such ties between
    differently coloured fragments even under the pure shift: the oracle counts them, and every kernel family must agree
    with it pixel for pixel -- the band kernel and k_mesh_rows (which settle a tie in two more passes over the row) and
    the global-key kernels (draw id in the z-buffer word, colour recomputed from it).  MDVT_DEBUG_SKIP=32 additionally
    makes the row kernels treat every pixel that received a second fragment as tied, so the extra passes run on every
    fold: the images must not change."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")          # the hooks below exist in the tuning build only (csrc/mdvt_internal.h)
    from metric_depth_video_toolbox_amd.depth_map_tools import compute_camera_matrix
    _lib, sr, synthetic = mods
    ties = 0
    for (W, H, t, kw, force_global) in ((256, 96, 180, {}, False), (256, 96, 60, dict(cull=2), False), (250, 64, 299, {}, False),
                                        (256, 96, 180, {}, True), (256, 64, 299, dict(dont_place_points_in_edges=True, remove_edges=True), False)):
        K = compute_camera_matrix(45.0, None, W, H)
        sc = synthetic.SyntheticScene(W, H, config_id=4)
        z = synthetic.contention_band(sc.depth_m(t), K[0, 0], 0.065, row0=H // 3, rows=H // 3)
        depth_rgb = synthetic.quantise_depth_to_rgb(z)
        _, color = sc.frame(t)
        if force_global:
            monkeypatch.setenv("MDVT_FORCE_GLOBAL", "1")
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)
        p = r.frame_params(xfov=45.0)
        orc.stats_reset()
        want = _oracle(orc, r, p, depth_rgb, color)
        ties += orc.stats()["depth_ties"]
        got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
        _compare(got, want, W, f"ties {W}x{H} t={t} {kw} global={force_global}")
        if force_global:     # ... and with every pixel that receives a second fragment marked as tied: the second rasteriser pass settles them all by draw id
            monkeypatch.setenv("MDVT_DEBUG_SKIP", "32")
            got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
            _compare(got, want, W, "ties, every overdrawn pixel through the second pass")
            monkeypatch.delenv("MDVT_DEBUG_SKIP")
        monkeypatch.delenv("MDVT_FORCE_GLOBAL", raising=False)
        r.close()
    assert ties >= 10, f"only {ties} exact depth ties in the oracle: the scenes no longer test the rule"
    monkeypatch.setenv("MDVT_DEBUG_SKIP", "32")
    for kw, (w, h) in ((dict(), (256, 64)), (dict(), (250, 37)), (dict(infill_mask=True), (256, 64)), (dict(cull=1), (256, 64))):
        depth_rgb, color = _scene(synthetic, w, h, seed=3)
        r = sr.StereoRerenderer(w, h, pupillary_distance=65, **kw)
        p = r.frame_params(xfov=45.0)
        got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
        _compare(got, _oracle(orc, r, p, depth_rgb, color), w, f"forced tie passes {kw} {w}x{h}")
        r.close()


def test_mesh_batch(mods, orc):
    _lib, sr, synthetic = mods
    W, H, N = 128, 80, 10
    d, c = synthetic.SyntheticScene(W, H, seed=4, n_fg=5).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
    params = [r.frame_params(xfov=42.0 + k) for k in range(N)]
    got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), params)
    for k in range(N):
        one = {key: v[k] for key, v in got.items()}
        _compare(one, _oracle(orc, r, params[k], d[k], c[k], want_depth=False), W, f"mesh batch frame {k}")
    r.close()


def test_mesh_full_hd_product_default(mods, orc):
    """1920x1080 through the product-default variant (mesh + edge filter + edge points)."""
    _lib, sr, synthetic = mods
    W, H = 1920, 1080
    depth_rgb, color = synthetic.SyntheticScene(W, H, config_id=2).frame(0)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
    p = r.frame_params(xfov=45.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, "mesh C2")
    r.close()


def test_codec_on_device(mods, orc, golden):
    from metric_depth_video_toolbox_amd import depth_frames_helper as dfh
    g = golden("codec")
    rgb = np.ascontiguousarray(np.tile(g["rnd_rgb"], (3, 5, 1)))
    for md, sc in ((100, 1.0), (20, 1.3938468501173518)):
        got = dfh.decode_rgb_depth_frame(torch.from_numpy(rgb).cuda(), md, True, depth_scale=sc).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), orc.decode_depth(rgb, md, sc).view(np.uint32))
    got = dfh.decode_rgb_depth_frame(torch.from_numpy(np.ascontiguousarray(g["kat_rgb"])).cuda(), 100, True).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), g["kat_dec_100"].view(np.uint32))
    enc_in = np.ascontiguousarray(g["enc_in"])
    bgr = dfh.encode_depth_frame(torch.from_numpy(enc_in).cuda(), 100).cpu().numpy()
    assert np.array_equal(bgr, g["enc_bgr"])                                   # the reference's own output
    rgb2 = dfh.encode_depth_frame(torch.from_numpy(enc_in).cuda(), 100, bgr=False).cpu().numpy()
    assert np.array_equal(rgb2, orc.encode_depth(enc_in, 100))
    odd = np.random.default_rng(1).uniform(-5, 120, (37, 251)).astype(np.float32)
    odd[3, 3] = np.nan
    assert np.array_equal(dfh.encode_depth_frame(torch.from_numpy(odd).cuda(), 100, bgr=False).cpu().numpy(),
                          orc.encode_depth(odd, 100))


@pytest.mark.parametrize("scene", ["a", "b", "c"])
@pytest.mark.parametrize("obo", [0, 1])
def test_edge_filter_matches_reference_goldens(mods, golden, scene, obo):
    """The device filter against the reference's own get_mesh_from_depth_map outputs."""
    _lib, sr, synthetic = mods
    g = golden("geometry")
    depth_rgb = np.ascontiguousarray(g[f"{scene}_depth_rgb"])
    H, W = depth_rgb.shape[:2]
    md = float(g[f"{scene}_max_depth"][0])
    xfov = {"a": 45.0, "b": 60.0, "c": 45.0}[scene]
    r = sr.StereoRerenderer(W, H, max_depth=md, master_xfov=xfov, render_as_pointcloud=not obo, remove_edges=True)
    p = r.frame_params(xfov=xfov)
    assert p.depth_scale == 1.0 and np.array_equal(_K(p), g[f"{scene}_K"])
    tri, unused = r.edge_filter(torch.from_numpy(depth_rgb).cuda(), p, of_by_one=bool(obo))
    assert np.array_equal(tri.cpu().numpy().astype(bool), g[f"{scene}_tri_invalid_obo{obo}"])
    assert np.array_equal(np.nonzero(unused.cpu().numpy())[0], g[f"{scene}_unused_obo{obo}"])
    r.close()


def test_edge_filter_full_size_matches_oracle(mods, orc):
    _lib, sr, synthetic = mods
    W, H = 640, 480
    depth_rgb, _ = synthetic.SyntheticScene(W, H, config_id=1).frame(0)
    r = sr.StereoRerenderer(W, H, remove_edges=True)
    p = r.frame_params(xfov=45.0)
    tri, unused = r.edge_filter(torch.from_numpy(depth_rgb).cuda(), p)
    d = orc.decode_depth(depth_rgb, 100, p.depth_scale)
    wt, wu, _ = orc.edge_filter(d, _K(p), True)
    assert wt.sum() > 1000
    assert np.array_equal(tri.cpu().numpy(), wt) and np.array_equal(unused.cpu().numpy(), wu)
    r.close()


def test_errors_are_reported_not_swallowed(mods):
    _lib, sr, synthetic = mods
    with pytest.raises(_lib.MdvtError) as e:
        _lib.Context(0, 0, 1)
    assert e.value.code == -1
    r = sr.StereoRerenderer(64, 48, render_as_pointcloud=True)
    with pytest.raises(ValueError):
        r.frame_params()
    bad = torch.zeros((48, 60, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        r.render(bad, bad, r.frame_params(xfov=45.0))
    p = r.frame_params(xfov=45.0)
    p.Krender[2] = 100.0           # render size != frame size (--vr180) is not built
    ok = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.MdvtError) as e:
        r.render(ok, ok, p)
    assert e.value.code == -3
    r.close()


@pytest.mark.parametrize("W,H,infill", [(3840, 40, True), (3840, 40, False), (4600, 24, True), (5000, 24, False)])
def test_mesh_wide_frames_use_compact_lds_vertices(mods, orc, W, H, infill):
    """Row widths whose 16-byte LDS vertex rows would exceed 160 KB take the 12-byte variant; beyond that (4600 px with
    edge points) the frame goes to the global-key kernels -- with the same pure-shift arithmetic, so nothing changes."""
    _lib, sr, synthetic = mods
    depth_rgb, color = _scene(synthetic, W, H, seed=W + H, n_fg=10)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=infill)
    p = r.frame_params(xfov=45.0)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"wide mesh {W}")
    r.close()


@pytest.mark.parametrize("W,H", [(20000, 4), (65535, 2), (12, 3000), (2, 32767)])
def test_extreme_frame_shapes(mods, orc, W, H):
    """The largest width / height a context takes, every mode: rows too wide for the LDS z-buffers (10 240 px for
    points) are rendered by the global-key kernels with the frame's own pure-shift arithmetic -- bit-exact as ever."""
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(W + H)
    for mesh in (False, True):
        for infill in (False, True):
            d = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            d[..., 0] = rng.integers(2, 40, (H, W))
            c = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
            r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=not mesh, infill_mask=infill)
            p = r.frame_params(xfov=60.0)
            got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_depth=True)
            _compare(got, _oracle(orc, r, p, d, c), W, f"{W}x{H} mesh={mesh} infill={infill}")
            r.close()
    with pytest.raises(_lib.MdvtError):
        _lib.Context(0, 65536, 2)
    with pytest.raises(_lib.MdvtError):
        _lib.Context(0, 2, 32768)


def test_global_key_kernels_keep_the_pure_shift_arithmetic(mods, orc, monkeypatch):
    """MDVT_FORCE_GLOBAL=1 routes pure-shift frames through the kernels of the general path (as too-wide frames are);
    the frame's arithmetic is its own, so every plane still equals the oracle's pure-shift evaluation."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")          # the hooks below exist in the tuning build only (csrc/mdvt_internal.h)
    _lib, sr, synthetic = mods
    monkeypatch.setenv("MDVT_FORCE_GLOBAL", "1")
    for W, H in ((250, 37), (64, 48)):
        depth_rgb, color = _scene(synthetic, W, H, seed=5)
        for mesh in (False, True):
            for infill in (False, True):
                r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=not mesh, infill_mask=infill)
                p = r.frame_params(xfov=45.0)
                got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True, want_seed=infill)
                op = orc.make_params(W, H, _K(p), ipd_m=0.065, depth_scale=p.depth_scale, mode=orc.MODE_MESH if mesh else orc.MODE_POINTS,
                                     remove_edges=r.remove_edges, edge_points=int(r.edge_points), key_rgb=r.key_rgb)
                assert op.general == 0
                want = orc.render_stereo(op, depth_rgb, color, want_depth=True, want_seed=infill)
                _compare({k: got[k] for k in ("sbs", "mask", "depth")}, want, W, f"forced global mesh={mesh} infill={infill}")
                if infill:
                    assert np.array_equal(got["seed"][:, :W].cpu().numpy(), want["left_seed"])
                    assert np.array_equal(got["seed"][:, W:].cpu().numpy(), want["right_seed"])
                r.close()


@pytest.mark.parametrize("kind", ["points_fast", "points_edges", "mesh", "points_general", "odd_width"])
def test_compacted_hole_mask_and_counts(mods, orc, kind):
    """1 bit/px hole mask (wavefront compaction) and per-eye hole counts agree with the byte mask."""
    _lib, sr, synthetic = mods
    W, H, N = (250, 37, 3) if kind == "odd_width" else (192, 108, 3)
    d, c = synthetic.SyntheticScene(W, H, seed=17, n_fg=6).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=kind != "mesh", infill_mask=kind == "points_edges")
    p = r.frame_params(xfov=45.0, convergence_distance=2.0 if kind == "points_general" else None)
    got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_maskbits=True, want_hole_counts=True)
    mask = got["mask"].cpu().numpy() > 0
    bits = got["maskbits"].cpu().numpy()
    counts = got["hole_counts"].cpu().numpy()
    for k in range(N):
        for eye, sl in ((0, slice(0, W)), (1, slice(W, 2 * W))):
            want = np.packbits(mask[k][:, sl], axis=1, bitorder="little")
            assert np.array_equal(bits[k, :, eye, :want.shape[1]], want), (kind, k, eye)
            assert counts[k, eye] == mask[k][:, sl].sum()
    one = {key: v[0] for key, v in got.items() if key in ("sbs", "mask")}
    _compare(one, _oracle(orc, r, p, d[0], c[0], want_depth=False), W, kind)
    r.close()


@pytest.mark.parametrize("shape", [(192, 108, 3), (1920, 21, 5), (1028, 7, 2), (2568, 33, 2), (1920, 1080, 3)])
def test_fused_mask_compaction_without_byte_mask(mods, shape):
    """The headline kernel with the compaction fused in and NO byte mask (want_mask=False): packed mask and counts equal those of a
    plain render's byte mask; the frame totals come out of the kernel's own accumulators (16 row classes + the frame word, left zero
    for the next launch: rendered three times, with a different clip the second time); every other path refuses NULL byte masks."""
    _lib, sr, synthetic = mods
    W, H, N = shape
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    clips = [synthetic.SyntheticScene(W, H, seed=s, n_fg=6).clip(N) for s in (17, 18, 17)]
    for d, c in clips:
        dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
        plain = r.render(dd, cc, p)
        got = r.render(dd, cc, p, want_maskbits=True, want_hole_counts=True, want_mask=False)
        assert "mask" not in got
        mask = plain["mask"].cpu().numpy() > 0
        bits, counts = got["maskbits"].cpu().numpy(), got["hole_counts"].cpu().numpy()
        assert np.array_equal(got["sbs"].cpu().numpy(), plain["sbs"].cpu().numpy())
        for k in range(N):
            for eye, sl in ((0, slice(0, W)), (1, slice(W, 2 * W))):
                want = np.packbits(mask[k][:, sl], axis=1, bitorder="little")
                assert np.array_equal(bits[k, :, eye, :want.shape[1]], want), (shape, k, eye)
                assert counts[k, eye] == mask[k][:, sl].sum(), (shape, k, eye)
    r.close()
    d, c = clips[0]
    for kw in (dict(render_as_pointcloud=False), dict(render_as_pointcloud=True, infill_mask=True)):
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)
        with pytest.raises(_lib.MdvtError) as e:
            r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), r.frame_params(xfov=45.0), want_maskbits=True, want_mask=False)
        assert e.value.code == -1 and "byte masks may be NULL only" in str(e.value)
        r.close()


def test_infill_using_normals_on_device(mods, orc, golden):
    """The HIP kernel against the reference's own outputs (golden) and against the oracle on a big case."""
    _lib, sr, synthetic = mods
    g = golden("infill")
    for scene in ("a", "b"):
        c, h, n = (torch.from_numpy(np.ascontiguousarray(g[f"{scene}_{k}"])).cuda() for k in ("color", "hole", "normal"))
        assert np.array_equal(sr.infill_using_normals(c, h, n).cpu().numpy(), g[f"{scene}_out"])
        assert np.array_equal(sr.infill_using_normals(c, h, n, max_steps=12).cpu().numpy(), g[f"{scene}_out_12"])
    rng = np.random.default_rng(5)
    W, H = 1283, 517
    color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    hole = rng.uniform(size=(H, W)) < 0.02
    for _ in range(40):
        x0, y0 = int(rng.integers(0, W - 80)), int(rng.integers(0, H - 60))
        hole[y0:y0 + int(rng.integers(5, 60)), x0:x0 + int(rng.integers(5, 80))] = True
    normal = rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)
    got = sr.infill_using_normals(torch.from_numpy(color).cuda(), torch.from_numpy(hole).cuda(), torch.from_numpy(normal).cuda())
    assert np.array_equal(got.cpu().numpy(), orc.infill_using_normals(color, hole, normal))


# ----------------------------------------------------------------------------------------------- raw ABI use
from footprint import raw_io as _raw_io  # noqa: E402  (moved into the footprint helper, unchanged)


@pytest.mark.parametrize("mode", ["points", "mesh"])
def test_raw_abi_with_padded_pitches_and_separate_eye_buffers(mods, orc, mode):
    """The C ABI takes arbitrary pitches: padded input rows, separate (non side-by-side) eye buffers, an
    unaligned pitch (-> the byte path), the single-frame entry point and a non-default stream."""
    import ctypes as C
    _lib, sr, synthetic = mods
    W, H = 120, 66
    depth_rgb, color = _scene(synthetic, W, H, seed=99)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=mode == "points", infill_mask=True)
    p = r.frame_params(xfov=45.0)
    want = _oracle(orc, r, p, depth_rgb, color)
    L = _lib.load()
    for in_pitch, out_pitch, m_pitch in ((3 * W, 3 * W, W), (3 * W + 20, 3 * W + 36, W + 8), (3 * W + 5, 3 * W + 7, W + 3)):
        dbuf = torch.zeros((H, in_pitch), dtype=torch.uint8, device="cuda")
        cbuf = torch.zeros((H, in_pitch), dtype=torch.uint8, device="cuda")
        dbuf[:, :3 * W] = torch.from_numpy(depth_rgb.reshape(H, 3 * W)).cuda()
        cbuf[:, :3 * W] = torch.from_numpy(color.reshape(H, 3 * W)).cuda()
        outs = {k: torch.full((H, out_pitch), 7, dtype=torch.uint8, device="cuda") for k in ("l", "r")}
        masks = {k: torch.full((H, m_pitch), 7, dtype=torch.uint8, device="cuda") for k in ("l", "r")}
        zl = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        zr = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        io = _raw_io(_lib, depth_rgb=dbuf.data_ptr(), depth_pitch=in_pitch, color_rgb=cbuf.data_ptr(), color_pitch=in_pitch,
                     left_rgb=outs["l"].data_ptr(), right_rgb=outs["r"].data_ptr(), rgb_pitch=out_pitch,
                     left_mask=masks["l"].data_ptr(), right_mask=masks["r"].data_ptr(), mask_pitch=m_pitch,
                     left_depth=zl.data_ptr(), right_depth=zr.data_ptr(), zout_pitch=4 * W)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        r.ctx.check(L.mdvt_render_stereo(r.ctx.handle, C.byref(p), C.byref(io), C.c_void_p(side.cuda_stream)))
        side.synchronize()
        for eye, k in (("left", "l"), ("right", "r")):
            assert np.array_equal(outs[k][:, :3 * W].cpu().numpy().reshape(H, W, 3), want[eye + "_rgb"]), (mode, in_pitch, eye)
            assert np.array_equal(masks[k][:, :W].cpu().numpy(), want[eye + "_mask"])
            assert (outs[k][:, 3 * W:] == 7).all() and (masks[k][:, W:] == 7).all(), "padding must stay untouched"
        assert np.array_equal(zl.cpu().numpy(), want["left_depth"]) and np.array_equal(zr.cpu().numpy(), want["right_depth"])
    r.close()


def test_parameter_cache_respects_changes_and_streams(mods, orc):
    """The library re-uses the device copy of identical parameter blocks; changing them (or the stream) must
    re-upload."""
    _lib, sr, synthetic = mods
    W, H = 128, 72
    depth_rgb, color = _scene(synthetic, W, H, seed=123)
    d, c = torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda()
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    for xfov in (45.0, 45.0, 50.0, 45.0):
        p = r.frame_params(xfov=xfov)
        _compare(r.render(d, c, p, want_depth=True), _oracle(orc, r, p, depth_rgb, color), W, f"cache xfov={xfov}")
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    p = r.frame_params(xfov=45.0)
    got = r.render(d, c, p, want_depth=True, stream=s2)
    s2.synchronize()
    _compare(got, _oracle(orc, r, p, depth_rgb, color), W, "cache other stream")
    r.close()


def test_invalid_arguments_return_codes(mods):
    import ctypes as C
    _lib, sr, synthetic = mods
    L = _lib.load()
    r = sr.StereoRerenderer(64, 48, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    buf = torch.zeros((48, 64 * 6), dtype=torch.uint8, device="cuda")
    ok = dict(depth_rgb=buf.data_ptr(), depth_pitch=192, color_rgb=buf.data_ptr(), color_pitch=192,
              left_rgb=buf.data_ptr(), right_rgb=buf.data_ptr() + 192, rgb_pitch=384,
              left_mask=buf.data_ptr(), right_mask=buf.data_ptr() + 64, mask_pitch=128)
    for bad in (dict(depth_rgb=None), dict(left_mask=None), dict(depth_pitch=100), dict(rgb_pitch=64), dict(mask_pitch=10)):
        io = _raw_io(_lib, **{**ok, **bad})
        assert L.mdvt_render_stereo(r.ctx.handle, C.byref(p), C.byref(io), None) == -1, bad
        assert len(L.mdvt_last_error(r.ctx.handle)) > 0
    io = _raw_io(_lib, **ok)
    assert L.mdvt_render_stereo_batch(r.ctx.handle, 0, C.byref(p), C.byref(io), None) == -1
    p2 = r.frame_params(xfov=45.0)
    p2.depth_scale = 0.0
    assert L.mdvt_render_stereo(r.ctx.handle, C.byref(p2), C.byref(io), None) == -1
    p3 = r.frame_params(xfov=45.0, transformation=np.arange(16.0).reshape(4, 4))       # not affine
    assert L.mdvt_render_stereo(r.ctx.handle, C.byref(p3), C.byref(io), None) == -3
    cfg = _lib.MdvtConfig(mode=7)
    assert L.mdvt_set_config(r.ctx.handle, C.byref(cfg)) == -1
    cfg = _lib.MdvtConfig(mode=0, edge_points=1, remove_edges=0, ipd_m=0.065, max_depth=100.0)
    assert L.mdvt_set_config(r.ctx.handle, C.byref(cfg)) == -1
    # (advisor r04) workspace_mib took over a reserved field: garbage from a caller built against the older header is refused
    cfg = _lib.MdvtConfig(mode=1, ipd_m=0.065, max_depth=100.0, workspace_mib=0xCDCDCDCD)
    assert L.mdvt_set_config(r.ctx.handle, C.byref(cfg)) == -1 and b"workspace_mib" in L.mdvt_last_error(r.ctx.handle)
    cfg = _lib.MdvtConfig(mode=1, ipd_m=0.065, max_depth=100.0, workspace_mib=1 << 20)
    assert L.mdvt_set_config(r.ctx.handle, C.byref(cfg)) == 0
    r.close()


def test_render_is_hip_graph_capturable(mods, orc):
    """Once the parameter block is staged (first call), a submission is a pure kernel launch and can be
    captured into a HIP graph and replayed on new input contents."""
    _lib, sr, synthetic = mods
    W, H, N = 256, 144, 4
    sc = synthetic.SyntheticScene(W, H, seed=77, n_fg=6)
    d0, c0 = sc.clip(N)
    d1, c1 = sc.clip(N, t0=10)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    d, c = torch.from_numpy(d0).cuda(), torch.from_numpy(c0).cuda()
    job = r.prepare(d, c, p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        job.launch(s)                       # stages the parameters
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            job.launch(torch.cuda.current_stream())
    for dd, cc in ((d0, c0), (d1, c1)):
        d.copy_(torch.from_numpy(dd).cuda()); c.copy_(torch.from_numpy(cc).cuda())
        torch.cuda.synchronize()
        job.results["sbs"].zero_(); job.results["mask"].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in range(N):
            one = {key: v[k] for key, v in job.results.items()}
            _compare(one, _oracle(orc, r, p, dd[k], cc[k], want_depth=False), W, f"graph replay frame {k}")
    r.close()


def sweep_cases(synthetic):
    """The seeded case generator of test_randomised_parity_sweep (also used by tests/dbg_sweep_case.py to replay one case).
    Soak runs: MDVT_SWEEP_SEED / MDVT_SWEEP_CASES widen the sweep (e.g. 400 cases per seed) without touching the default;
    MDVT_SWEEP_SIZES="1920x1080,1280x720" gives a full-size soak (the oracle takes seconds per case)."""
    import os
    rng = np.random.default_rng(int(os.environ.get("MDVT_SWEEP_SEED", "20260927")))
    sizes = [(2, 2), (3, 2), (4, 4), (5, 3), (8, 8), (17, 9), (36, 20), (61, 33), (64, 32), (100, 31), (128, 16), (200, 12)]
    n_cases = int(os.environ.get("MDVT_SWEEP_CASES", "60"))
    soak = n_cases > 60 or "MDVT_SWEEP_SIZES" in os.environ
    if soak:
        sizes += [(320, 200), (257, 129), (96, 96), (512, 9), (40, 300)]
    if "MDVT_SWEEP_SIZES" in os.environ:
        sizes = [tuple(int(v) for v in t.split("x")) for t in os.environ["MDVT_SWEEP_SIZES"].split(",")]
    for case in range(n_cases):
        W, H = sizes[int(rng.integers(len(sizes)))]
        mesh = bool(rng.integers(2))
        infill = bool(rng.integers(2))
        no_pts = bool(rng.integers(4) == 0)
        ipd = int(rng.choice([0, 1, 30, 63, 65, 120, 400]))
        xfov = float(rng.choice([20.0, 45.0, 60.0, 90.0, 120.0]))
        master = float(rng.choice([25.0, 45.0, 70.0]))
        max_depth = int(rng.choice([5, 20, 100, 655]))
        kind = int(rng.integers(4))                      # 0 pure, 1 convergence, 2 pose, 3 both
        depth_rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        style = int(rng.integers(8 if soak else 4))
        if style == 3 and mesh and W * H > 500_000:
            style = 4            # white-noise depth at full size: every triangle spans the frame and the ORACLE needs ~half an hour per frame
        if soak and rng.integers(4) == 0:                # soak only: extreme camera scalars
            ipd = int(rng.choice([2000, 7, 250]))
            xfov = float(rng.choice([5.0, 150.0, 170.0, 33.3]))
        if style == 4:                                   # foreground rectangles over a far plane (typical scene structure)
            code = np.full((H, W), int(rng.integers(3000, 60000)), np.uint32)
            for _ in range(int(rng.integers(1, 6))):
                x0, y0 = int(rng.integers(W)), int(rng.integers(H))
                code[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = int(rng.integers(50, 3000))
            depth_rgb[..., 0] = (code >> 8) & 0xFF; depth_rgb[..., 2] = code & 0xFF
        elif style == 5:                                 # one-code noise on a slope: z ties and 1-LSB steps everywhere
            code = (int(rng.integers(300, 40000)) + np.arange(W)[None, :] // 3 + rng.integers(0, 2, (H, W))).astype(np.uint32)
            depth_rgb[..., 0] = (code >> 8) & 0xFF; depth_rgb[..., 2] = code & 0xFF
        elif style == 6:                                 # alternating near / far columns or rows: maximal folding
            near, far = int(rng.integers(20, 400)), int(rng.integers(5000, 65000))
            stripes = (np.arange(W)[None, :] if rng.integers(2) else np.arange(H)[:, None]) // int(rng.integers(1, 4)) % 2
            code = np.where(np.broadcast_to(stripes, (H, W)) == 0, near, far).astype(np.uint32)
            depth_rgb[..., 0] = (code >> 8) & 0xFF; depth_rgb[..., 2] = code & 0xFF
        elif style == 7:                                 # the far end of the code range
            depth_rgb[..., 0] = 255; depth_rgb[..., 2] = rng.integers(200, 256, (H, W))
        if style == 0:                                   # smooth plane + a step
            code = (2000 + 40 * np.arange(W)[None, :] + 7 * np.arange(H)[:, None]).astype(np.uint32)
            code[:, W // 2:] //= 3
            depth_rgb[..., 0] = (code >> 8) & 0xFF
            depth_rgb[..., 2] = code & 0xFF
        elif style == 1:                                 # very near content: huge disparities, near-plane rejects
            depth_rgb[..., 0] = 0
            depth_rgb[..., 2] = rng.integers(0, 4, (H, W))
        elif style == 2:                                 # constant depth
            depth_rgb[..., 0] = 3
            depth_rgb[..., 2] = 77
        color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if rng.integers(2):
            color[rng.integers(H), rng.integers(W)] = (0, 255, 0) if infill else (0, 0, 0)
        T = None
        if kind >= 2:
            T = synthetic.synthetic_pose_track(64)[int(rng.integers(1, 64))]
            T[:3, 3] *= float(rng.choice([1.0, 20.0]))
            if soak and rng.integers(3) == 0:            # a big rotation about a random axis, possibly looking backwards
                ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
                ang = float(rng.choice([0.3, 1.0, 1.5708, 3.1])); Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
                R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
                T = T.copy(); T[:3, :3] = R @ T[:3, :3]
        conv_d = float(rng.uniform(0.3, 8.0)) if kind in (1, 3) else None
        if soak and conv_d is not None and rng.integers(5) == 0:
            conv_d = float(rng.choice([0.02, 0.05, 500.0]))
        yield dict(case=case, W=W, H=H, mesh=mesh, infill=infill, no_pts=no_pts, ipd=ipd, xfov=xfov, master=master, max_depth=max_depth,
                   kind=kind, style=style, depth_rgb=depth_rgb, color=color, T=T, conv_d=conv_d)


def test_randomised_parity_sweep(mods, orc):
    """Seeded random sweep over sizes (incl. tiny / odd), camera scalars, modes, flags, poses and
    degenerate depth content; every output plane must equal the oracle bit for bit."""
    _lib, sr, synthetic = mods
    for cs in sweep_cases(synthetic):
        W, H, mesh, infill, no_pts, ipd, xfov, max_depth, T = (cs[k] for k in ("W", "H", "mesh", "infill", "no_pts", "ipd", "xfov", "max_depth", "T"))
        depth_rgb, color = cs["depth_rgb"], cs["color"]
        r = sr.StereoRerenderer(W, H, pupillary_distance=ipd, max_depth=max_depth, master_xfov=cs["master"],
                                render_as_pointcloud=not mesh, infill_mask=infill, dont_place_points_in_edges=no_pts)
        p = r.frame_params(xfov=xfov, convergence_distance=cs["conv_d"], transformation=T)
        want_seed = infill and H >= 3 and W >= 3
        got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True, want_seed=want_seed,
                       want_maskbits=True, want_hole_counts=True)
        tag = f"sweep#{cs['case']} {W}x{H} mesh={mesh} infill={infill} no_pts={no_pts} ipd={ipd} xfov={xfov} md={max_depth} kind={cs['kind']} style={cs['style']}"
        op = orc.make_params(W, H, _K(p), ipd_m=ipd / 1000, max_depth=max_depth, depth_scale=p.depth_scale,
                             mode=orc.MODE_MESH if mesh else orc.MODE_POINTS, remove_edges=r.remove_edges, edge_points=int(r.edge_points),
                             conv_angle=p.convergence_angle, T=T, key_rgb=r.key_rgb)
        want = orc.render_stereo(op, depth_rgb, color, want_depth=True, want_seed=want_seed)
        _compare({k: got[k] for k in ("sbs", "mask", "depth")}, want, W, tag)
        # the packed mask and the hole counts (fused into the headline kernel, a post-pass everywhere else) say what the byte mask says
        mk, bits, counts = got["mask"].cpu().numpy() > 0, got["maskbits"].cpu().numpy(), got["hole_counts"].cpu().numpy()
        for eye, sl in ((0, slice(0, W)), (1, slice(W, 2 * W))):
            pk = np.packbits(mk[:, sl], axis=1, bitorder="little")
            assert np.array_equal(bits[:, eye, :pk.shape[1]], pk) and int(counts[eye]) == int(mk[:, sl].sum()), tag + " packed mask / counts"
        if want_seed:            # the infill-mask chain on whatever seeds this case produced
            fin = r.finish_infill_mask_sbs(got["seed"]).cpu().numpy()
            for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                assert np.array_equal(got["seed"][:, sl].cpu().numpy(), want[eye + "_seed"]), tag + " seed " + eye
                assert np.array_equal(fin[:, sl], orc.finish_infill_mask(want[eye + "_seed"], max_rounds=256)[0]), tag + " finish " + eye
        r.close()


def batch_sweep_cases(synthetic):
    """Seeded generator of MULTI-FRAME calls (the single-frame sweep above never submits one): 2 ... 40 frames per call, one
    renderer configuration per call, every frame with its own depth content and its own kind -- pure shift, convergence, pose or
    both -- in runs long enough that the posed / converged paths split into several launch sets on two banks of workspace slots
    (mdvt_render_stereo_batch); a small `workspace_mib` makes the mesh path's sets short.  MDVT_SWEEP_SEED / MDVT_BATCH_CASES
    widen it for tools/soak.py."""
    import os
    rng = np.random.default_rng(int(os.environ.get("MDVT_SWEEP_SEED", "20260927")) + 7_000_003)
    sizes = [(8, 8), (17, 9), (36, 20), (61, 33), (64, 32), (100, 31), (128, 16), (200, 12), (96, 96), (257, 129), (320, 200)]
    for case in range(int(os.environ.get("MDVT_BATCH_CASES", "24"))):
        W, H = sizes[int(rng.integers(len(sizes)))]
        N = int(rng.integers(2, 41))
        if W * H > 20000:
            N = min(N, 12)                                   # (the oracle's share)
        mesh, infill, no_pts = bool(rng.integers(4) != 0), bool(rng.integers(2)), bool(rng.integers(4) == 0)
        ipd = int(rng.choice([1, 30, 63, 65, 120]))
        xfov = float(rng.choice([45.0, 60.0, 90.0, 120.0]))
        max_depth = int(rng.choice([20, 100]))
        # slots one launch set may take: 0 = the library's default budget; else a budget of 2 ... 6 slots (mesh, posed / converged)
        slots = int(rng.choice([0, 2, 3, 4, 6]))
        per_slot = W * H * (16 + 48 + 32 + 24 + 3)
        ws_mib = 0 if slots == 0 else max(1, -(-slots * per_slot // (1 << 20)))
        layout = int(rng.integers(4))                        # 0: one kind throughout, 1: random per frame, 2: two long runs, 3: general except a pure frame or two
        kinds = []
        base = int(rng.integers(1, 4))
        for f in range(N):
            if layout == 0: k = base
            elif layout == 1: k = int(rng.integers(4))
            elif layout == 2: k = base if f < N // 2 else (base % 3) + 1
            else: k = 0 if rng.integers(8) == 0 else base
            kinds.append(k)
        d = np.zeros((N, H, W, 3), np.uint8)
        for f in range(N):
            style = int(rng.integers(4))
            if style == 0:                                   # foreground rectangles over a far plane
                code = np.full((H, W), int(rng.integers(3000, 60000)), np.uint32)
                for _ in range(int(rng.integers(1, 6))):
                    x0, y0 = int(rng.integers(W)), int(rng.integers(H))
                    code[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = int(rng.integers(50, 3000))
            elif style == 1:                                 # one-code noise on a slope: ties and 1-LSB steps
                code = (int(rng.integers(300, 40000)) + np.arange(W)[None, :] // 3 + rng.integers(0, 2, (H, W))).astype(np.uint32)
            elif style == 2:                                 # near / far stripes: folding, large triangles
                near, far = int(rng.integers(20, 400)), int(rng.integers(5000, 65000))
                stripes = (np.arange(W)[None, :] if rng.integers(2) else np.arange(H)[:, None]) // int(rng.integers(1, 4)) % 2
                code = np.where(np.broadcast_to(stripes, (H, W)) == 0, near, far).astype(np.uint32)
            else:                                            # smooth plane + a step
                code = (2000 + 40 * np.arange(W)[None, :] + 7 * np.arange(H)[:, None]).astype(np.uint32)
                code[:, W // 2:] //= 3
            code = np.minimum(code, 65535)
            d[f, ..., 0] = (code >> 8) & 0xFF; d[f, ..., 1] = d[f, ..., 0]; d[f, ..., 2] = code & 0xFF
        c = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        track = synthetic.synthetic_pose_track(64)
        Ts = [track[int(rng.integers(1, 64))] if k >= 2 else None for k in kinds]
        convs = [float(rng.uniform(0.5, 8.0)) if k in (1, 3) else None for k in kinds]
        if layout == 0 and base == 1 and rng.integers(2):
            convs = [convs[0]] * N                           # a clip-constant convergence, as movie_2_3D.py passes it
        yield dict(case=case, W=W, H=H, N=N, mesh=mesh, infill=infill, no_pts=no_pts, ipd=ipd, xfov=xfov, max_depth=max_depth,
                   ws_mib=ws_mib, kinds=kinds, depth_rgb=d, color=c, Ts=Ts, convs=convs)


def test_randomised_batch_sweep(mods, orc):
    """Multi-frame calls against the oracle frame by frame: sbs, mask, depth planes and seed images; each call twice (slot parities)."""
    _lib, sr, synthetic = mods
    for cs in batch_sweep_cases(synthetic):
        W, H, N = cs["W"], cs["H"], cs["N"]
        r = sr.StereoRerenderer(W, H, pupillary_distance=cs["ipd"], max_depth=cs["max_depth"], render_as_pointcloud=not cs["mesh"],
                                infill_mask=cs["infill"], dont_place_points_in_edges=cs["no_pts"], workspace_mib=cs["ws_mib"])
        ps = [r.frame_params(xfov=cs["xfov"], convergence_distance=cs["convs"][f], transformation=cs["Ts"][f]) for f in range(N)]
        want_seed = cs["infill"] and H >= 3 and W >= 3
        dt, ct = torch.from_numpy(cs["depth_rgb"]).cuda(), torch.from_numpy(cs["color"]).cuda()
        tag0 = (f"batch#{cs['case']} {W}x{H} x {N} mesh={cs['mesh']} infill={cs['infill']} no_pts={cs['no_pts']} ipd={cs['ipd']} xfov={cs['xfov']} "
                f"md={cs['max_depth']} ws_mib={cs['ws_mib']} kinds={''.join(map(str, cs['kinds']))}")
        for rep in range(2):
            got = r.render(dt, ct, ps, want_depth=True, want_seed=want_seed)
            for f in range(N):
                op = orc.make_params(W, H, _K(ps[f]), ipd_m=cs["ipd"] / 1000, max_depth=cs["max_depth"], depth_scale=ps[f].depth_scale,
                                     mode=orc.MODE_MESH if cs["mesh"] else orc.MODE_POINTS, remove_edges=r.remove_edges,
                                     edge_points=int(r.edge_points), conv_angle=ps[f].convergence_angle, T=cs["Ts"][f], key_rgb=r.key_rgb)
                want = orc.render_stereo(op, cs["depth_rgb"][f], cs["color"][f], want_depth=True, want_seed=want_seed) if rep == 0 else wants[f]
                if rep == 0:
                    if f == 0: wants = []
                    wants.append(want)
                tag = f"{tag0} call {rep} frame {f}"
                _compare({k: got[k][f] for k in ("sbs", "mask", "depth")}, want, W, tag)
                if want_seed:
                    sd = got["seed"][f].cpu().numpy()
                    for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                        assert np.array_equal(sd[:, sl], want[eye + "_seed"]), tag + " seed " + eye
        r.close()


def test_mark_lower_side_on_device(mods, orc, golden):
    from metric_depth_video_toolbox_amd import infill_common
    g = golden("infill")
    for scene in ("m1", "m2"):
        img = torch.from_numpy(np.ascontiguousarray(g[f"{scene}_img"])).cuda()
        assert np.array_equal(infill_common.mark_lower_side(img).cpu().numpy(), g[f"{scene}_out"])
        assert np.array_equal(infill_common.mark_lower_side(img, max_steps=8).cpu().numpy(), g[f"{scene}_out_8"])
    rng = np.random.default_rng(11)
    big = np.zeros((300, 501, 3), np.uint8)
    for _ in range(60):
        x0, y0 = int(rng.integers(0, 460)), int(rng.integers(0, 270))
        big[y0:y0 + int(rng.integers(3, 30)), x0:x0 + int(rng.integers(3, 40))] = rng.integers(1, 256, 3)
    assert np.array_equal(infill_common.mark_lower_side(torch.from_numpy(big).cuda()).cpu().numpy(), orc.mark_lower_side(big))


@pytest.mark.parametrize("mode", ["mesh", "points"])
@pytest.mark.parametrize("kind", ["pure", "convergence", "pose", "no_edge_points"])
def test_infill_mask_seed_image(mods, orc, mode, kind):
    """The infill-mask seed (sr:787-803, just before cv2.inpaint): key colour / border normals / removed-vertex
    normals carried through the eye transform, against the oracle (whose vertex normals are pinned bit-exactly
    by the reference's get_mesh_from_depth_map goldens)."""
    _lib, sr, synthetic = mods
    W, H = 176, 100
    depth_rgb, color = _scene(synthetic, W, H, seed=314, n_fg=7)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=mode == "points", infill_mask=True,
                            dont_place_points_in_edges=kind == "no_edge_points")
    T = synthetic.synthetic_pose_track(50)[41] if kind == "pose" else None
    p = r.frame_params(xfov=45.0, convergence_distance=2.2 if kind == "convergence" else None, transformation=T)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_seed=True)
    op = orc.make_params(W, H, _K(p), ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale,
                         mode=orc.MODE_POINTS if mode == "points" else orc.MODE_MESH, remove_edges=True,
                         edge_points=r.edge_points, conv_angle=p.convergence_angle, T=T, key_rgb=(0, 255, 0))
    want = orc.render_stereo(op, depth_rgb, color, want_seed=True)
    _compare({k: v for k, v in got.items() if k != "seed"}, want, W, f"seed {mode}/{kind}")
    seed = got["seed"].cpu().numpy()
    for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
        s, ws = seed[:, sl], want[eye + "_seed"]
        assert np.array_equal(s, ws), f"{mode}/{kind} {eye} seed differs at {int(np.any(s != ws, axis=-1).sum())} px"
        hole = want[eye + "_mask"] > 0
        assert not s[~hole].any() and np.all(np.any(s[hole] != 0, axis=-1))       # black <=> not a hole
        if kind != "no_edge_points":
            is_key = np.all(s == np.array([0, 255, 0], np.uint8), axis=-1)
            assert (hole & ~is_key).sum() > 20, "some holes must carry normals"
    r.close()


@pytest.mark.parametrize("inband", [False, True])
@pytest.mark.parametrize("size", [(250, 37), (256, 64), (1280, 24), (2560, 20), (3840, 12)])
def test_mesh_edge_points_after_the_row_kernel(mods, orc, monkeypatch, size, inband):
    """Pure-shift mesh frames with edge points: the row kernel renders without them and k_edge_rows_pure places them afterwards
    (a workgroup per 8 scanlines; 1, 2 or 4 four-column groups per thread, or column by column when the rows are not
    dword-addressable -- one size per variant), k_edge_rows_exact on the scanlines whose points move a row.  Images, masks, depth
    planes and seed images against the oracle; and the same with MDVT_EDGE_INBAND=1 (tuning build), which keeps the points
    inside the row kernels as until r04 -- the A/B the choice was made on."""
    _lib, sr, synthetic = mods
    if inband:
        monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")
        monkeypatch.setenv("MDVT_EDGE_INBAND", "1")
    W, H = size
    for seed, xfov in ((11, 45.0), (12, 97.3)):
        depth_rgb, color = _scene(synthetic, W, H, seed=seed, n_fg=9)
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
        p = r.frame_params(xfov=xfov)
        got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_seed=True, want_depth=True)
        op = orc.make_params(W, H, _K(p), ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale, mode=orc.MODE_MESH, remove_edges=True,
                             edge_points=r.edge_points, conv_angle=0.0, T=None, key_rgb=(0, 255, 0))
        want = orc.render_stereo(op, depth_rgb, color, want_seed=True, want_depth=True)
        _compare({k: v for k, v in got.items() if k != "seed"}, want, W, f"edge points after {W}x{H} inband={inband}")
        seed_img = got["seed"].cpu().numpy()
        painted = 0
        for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
            assert np.array_equal(seed_img[:, sl], want[eye + "_seed"]), f"{W}x{H} {eye} seed, inband={inband}"
            hole = want[eye + "_mask"] > 0
            painted += int((hole & np.any(want[eye + "_rgb"] != 0, axis=-1)).sum())
        assert painted > 0, "no edge point landed in a hole: the scene no longer tests the pass"
        r.close()


@pytest.mark.parametrize("rows", [1, 2, 3, 5, 8])
def test_mesh_band_heights(mods, orc, monkeypatch, rows):
    """k_mesh_band renders bands of 1..8 scanlines per workgroup, chosen by the size of the launch (a single frame gets short
    bands so that it still fills the chip, a launch of 32 frames 8): every height must give the same images.  MDVT_MESH_BAND
    (tuning build) pins the height; plain mesh and mesh + --infill_mask (edge filter, edge points afterwards, seed image), an
    image height that is no multiple of any band height, depth planes."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")
    monkeypatch.setenv("MDVT_MESH_BAND", str(rows))
    _lib, sr, synthetic = mods
    W, H = 256, 77
    for kw in (dict(), dict(infill_mask=True), dict(cull=1)):
        depth_rgb, color = _scene(synthetic, W, H, seed=21 + rows, n_fg=8)
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)
        p = r.frame_params(xfov=60.0)
        seed = bool(kw.get("infill_mask"))
        got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True, want_seed=seed)
        op = orc.make_params(W, H, _K(p), ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale, mode=orc.MODE_MESH,
                             remove_edges=r.remove_edges, edge_points=r.edge_points, conv_angle=0.0, T=None, key_rgb=(0, 255, 0),
                             cull=kw.get("cull", 0))
        want = orc.render_stereo(op, depth_rgb, color, want_depth=True, want_seed=seed)
        _compare({k: v for k, v in got.items() if k != "seed"}, want, W, f"band height {rows} {kw}")
        if seed:
            for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                assert np.array_equal(got["seed"][:, sl].cpu().numpy(), want[eye + "_seed"]), f"band height {rows} seed {eye}"
        r.close()


def test_mesh_band_height_follows_the_launch(mods, orc):
    """... and without the hook (product library): launches of 1, 3, 9 and 40 frames of 256 x 270 take bands of 1, 1, 1 and 4
    scanlines (launch_mesh_band); the same clip in every grouping gives the same frames."""
    _lib, sr, synthetic = mods
    W, H, N = 256, 270, 40
    d, c = synthetic.SyntheticScene(W, H, seed=9, n_fg=6).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65)
    ps = [r.frame_params(xfov=45.0) for _ in range(N)]
    dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    whole = r.render(dd, cc, ps)
    for lo, hi in ((0, 1), (1, 4), (4, 13)):
        part = r.render(dd[lo:hi], cc[lo:hi], ps[lo:hi] if hi - lo > 1 else ps[lo])
        assert torch.equal(part["sbs"], whole["sbs"][lo:hi]) and torch.equal(part["mask"], whole["mask"][lo:hi]), (lo, hi)
    for k in (0, 17, 39):
        _compare({"sbs": whole["sbs"][k], "mask": whole["mask"][k]}, _oracle(orc, r, ps[k], d[k], c[k], want_depth=False), W, f"frame {k} of 40")
    r.close()


@pytest.mark.parametrize("case", [dict(W=250, H=61, N=9, mib=8, kw=dict()), dict(W=320, H=64, N=14, mib=14, kw=dict(cull=1)),
                                  dict(W=128, H=80, N=33, mib=9, kw=dict(infill_mask=True)), dict(W=640, H=48, N=10, mib=16, kw=dict(remove_edges=True)),
                                  dict(W=250, H=61, N=11, mib=0, kw=dict(render_as_pointcloud=True)),
                                  dict(W=256, H=64, N=9, mib=0, kw=dict(render_as_pointcloud=True, infill_mask=True))])
def test_two_banks_on_other_shapes(mods, orc, case):
    """The same on other frame shapes, set lengths and flag sets (a width that is no multiple of four, odd set counts, a last set
    shorter than the others), and for points on the general path (banks of two frames): every frame of the batch against the
    oracle, twice (both parities of the z-key slots)."""
    _lib, sr, synthetic = mods
    W, H, N = case["W"], case["H"], case["N"]
    d, c = synthetic.SyntheticScene(W, H, seed=W + N, n_fg=5).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, workspace_mib=case["mib"], **case["kw"])
    T = synthetic.synthetic_pose_track(N + 8)
    ps = [r.frame_params(xfov=50.0, convergence_distance=None if k % 2 else 2.2, transformation=T[k + 2] if k % 2 else None) for k in range(N)]
    dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    for rep in range(2):
        got = r.render(dd, cc, ps, want_depth=True)
        for k in range(N):
            want = _oracle(orc, r, ps[k], d[k], c[k], T=T[k + 2] if k % 2 else None)
            _compare({key: v[k] for key, v in got.items()}, want, W, f"banks {W}x{H} frame {k} of {N}, pass {rep}")
    r.close()


def test_converged_mesh_launch_sets_on_two_banks(mods, orc):
    """A posed / converged mesh batch of more than one launch set is rendered set by set on two halves of the workspace slots and two
    streams, a set starting when the one before it has projected its vertices (mdvt_render_stereo_batch).  21 frames under a
    19 MiB budget are launch sets of 3 frames per bank here: every output plane must be what the same frames give one by one (single
    sets, no banks), and what the oracle gives; with hole counts or packed masks requested the sets stay on one stream."""
    _lib, sr, synthetic = mods
    W, H, N = 256, 96, 21
    d, c = synthetic.SyntheticScene(W, H, seed=12, n_fg=6).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True, workspace_mib=19)
    T = synthetic.synthetic_pose_track(N + 5)
    ps = [r.frame_params(xfov=45.0, convergence_distance=2.0 + 0.05 * k, transformation=T[k + 3] if k % 3 == 0 else None) for k in range(N)]
    dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    whole = r.render(dd, cc, ps, want_depth=True, want_seed=True)
    again = r.render(dd, cc, ps, want_depth=True, want_seed=True)            # (the other parity of every slot)
    counted = r.render(dd, cc, ps, want_depth=True, want_seed=True, want_hole_counts=True, want_maskbits=True)
    torch.cuda.synchronize()
    for key in ("sbs", "mask", "depth", "seed"):
        assert torch.equal(whole[key], again[key]) and torch.equal(whole[key], counted[key]), key
    for k in range(N):
        one = r.render(dd[k], cc[k], ps[k], want_depth=True, want_seed=True)
        for key in ("sbs", "mask", "depth", "seed"):
            assert torch.equal(one[key], whole[key][k]), (key, k)
    for k in (0, 10, 11, 20):
        op = orc.make_params(W, H, _K(ps[k]), ipd_m=0.065, max_depth=100, depth_scale=ps[k].depth_scale, mode=orc.MODE_MESH, remove_edges=True,
                             edge_points=r.edge_points, conv_angle=ps[k].convergence_angle, T=T[k + 3] if k % 3 == 0 else None, key_rgb=(0, 255, 0))
        want = orc.render_stereo(op, d[k], c[k], want_depth=True, want_seed=True)
        _compare({"sbs": whole["sbs"][k], "mask": whole["mask"][k], "depth": whole["depth"][k]}, want, W, f"banks, frame {k}")
        for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
            assert np.array_equal(whole["seed"][k][:, sl].cpu().numpy(), want[eye + "_seed"]), (k, eye)
    r.close()


@pytest.mark.parametrize("tmax,tmin", [(5, 0), (5.0, 0.5), (12.5, 1.0)])
def test_touchly_depth_plane(mods, tmax, tmin):
    """sr:549-551 evaluated literally with NumPy (the reference's expression is script-level code) vs the kernel,
    plus the --touchly1 fast-path frame: vconcat([colour, plane]) (sr:548-552)."""
    _lib, sr, synthetic = mods
    from metric_depth_video_toolbox_amd import depth_frames_helper as dfh
    W, H = 250, 61
    depth_rgb, color = _scene(synthetic, W, H, seed=8)
    d_t = dfh.decode_rgb_depth_frame(torch.from_numpy(depth_rgb).cuda(), 100, True, depth_scale=1.3938468501173518)
    depth = d_t.cpu().numpy()
    for zero_is_far in (False, True):
        d8 = np.rint(np.maximum(0, np.minimum(depth, tmax) - tmin) * (255 / (tmax - tmin))).astype(np.uint8)
        if zero_is_far:
            d8[d8 == 0] = 255
        want = np.repeat((255 - d8)[..., np.newaxis], 3, axis=-1)
        got = sr.touchly_depth(d_t, tmax, tmin, zero_is_far=zero_is_far).cpu().numpy()
        assert np.array_equal(got, want)
    frame = torch.cat([torch.from_numpy(color).cuda(), sr.touchly_depth(d_t, tmax, tmin)], dim=0)       # cv2.vconcat
    assert tuple(frame.shape) == (2 * H, W, 3)


def test_bench_workload_is_bit_exact_and_deterministic(mods, orc):
    """The 32 host-generated frames of the workload bench.py times (1920x1080, points mode, 65 mm, xfov 45, one batched
    launch; the bench's step is 128 frames -- these 32 plus device-rolled copies, see
    test_bench_step_of_128_frames_with_rolled_copies): every frame equals the oracle bit for bit, two launches agree
    (atomic order does not matter), and a frame rendered inside the batch equals the same frame rendered alone."""
    _lib, sr, synthetic = mods
    W, H, N = 1920, 1080, 32
    d, c = synthetic.SyntheticScene(W, H, config_id=2).clip(N)
    dt, ct = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    a = r.render(dt, ct, p, want_hole_counts=True)
    sbs1, mask1 = a["sbs"].clone(), a["mask"].clone()
    b = r.render(dt, ct, p)
    assert torch.equal(sbs1, b["sbs"]) and torch.equal(mask1, b["mask"])
    counts = a["hole_counts"].cpu().numpy()
    K = _K(p)
    op = orc.make_params(W, H, K, ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale, mode=orc.MODE_POINTS)
    sbs, mask = sbs1.cpu().numpy(), mask1.cpu().numpy()
    for k in range(N):
        want = orc.render_stereo(op, d[k], c[k])
        assert np.array_equal(mask[k][:, :W], want["left_mask"]) and np.array_equal(mask[k][:, W:], want["right_mask"]), k
        assert np.array_equal(sbs[k][:, :W], want["left_rgb"]) and np.array_equal(sbs[k][:, W:], want["right_rgb"]), k
        assert counts[k, 0] == (want["left_mask"] > 0).sum() and counts[k, 1] == (want["right_mask"] > 0).sum()
        # a splat maps every source to at most one target per eye
        assert (want["left_mask"] == 0).sum() <= W * H
    one = r.render(dt[17], ct[17], p)
    assert torch.equal(one["sbs"], sbs1[17]) and torch.equal(one["mask"], mask1[17])
    r.close()


def test_bench_step_of_128_frames_with_rolled_copies(mods, orc):
    """bench.py's headline step literally: 128 frames of 1920x1080 in ONE launch, frames 32.. being the first 32 rolled by
    whole pixels on the device (bench.py main()).  Frames from every quarter of the batch -- index >= 32 included -- are
    compared with the oracle on the same (host-rolled) inputs."""
    _lib, sr, synthetic = mods
    W, H, N, NH = 1920, 1080, 128, 32
    d, c = synthetic.SyntheticScene(W, H, config_id=2).clip(NH)
    dt = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    ct = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    dt[:NH], ct[:NH] = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    for k in range(NH, N):
        sh = (7 * (k // NH), 13 * (k // NH))
        dt[k] = torch.roll(dt[k % NH], shifts=sh, dims=(0, 1))
        ct[k] = torch.roll(ct[k % NH], shifts=sh, dims=(0, 1))
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True)
    p = r.frame_params(xfov=45.0)
    got = r.render(dt, ct, r.pack_params([p] * N, N))
    op = orc.make_params(W, H, _K(p), ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale, mode=orc.MODE_POINTS)
    for k in (5, 37, 70, 101, 127):
        sh = (7 * (k // NH), 13 * (k // NH))
        dk, ck = np.roll(d[k % NH], sh, axis=(0, 1)), np.roll(c[k % NH], sh, axis=(0, 1))
        assert np.array_equal(dt[k].cpu().numpy(), dk)
        want = orc.render_stereo(op, np.ascontiguousarray(dk), np.ascontiguousarray(ck))
        _compare({"sbs": got["sbs"][k], "mask": got["mask"][k]}, want, W, f"128-frame step, frame {k}")
    r.close()


@pytest.mark.parametrize("variant", ["mesh", "product_default"])
def test_bench_extras_at_full_hd(mods, orc, variant):
    """What bench.py's `extra` object times, at the size it times it (1920x1080, 65 mm, xfov 45), frames inside a batch:
    `mesh` = plain mesh mode, pure shift (k_mesh_band<0, 512>); `product_default` = mesh + --infill_mask + convergence at
    2.5 m (movie_2_3D.py:433-445) with the seed image.  LDS ring sizing, queue segments and launch-set chunking all depend
    on W and H, so the small-frame tests do not stand in for this one."""
    _lib, sr, synthetic = mods
    W, H, N = 1920, 1080, 3
    d, c = synthetic.SyntheticScene(W, H, config_id=2).clip(N, t0=11)
    kw = dict(infill_mask=True) if variant == "product_default" else {}
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)
    p = r.frame_params(xfov=45.0, convergence_distance=2.5 if variant == "product_default" else None)
    seed = variant == "product_default"
    got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), [p] * N, want_depth=True, want_seed=seed)
    for k in (0, 2):
        op = orc.make_params(W, H, _K(p), ipd_m=0.065, max_depth=100, depth_scale=p.depth_scale, mode=orc.MODE_MESH,
                             remove_edges=r.remove_edges, edge_points=int(r.edge_points), conv_angle=p.convergence_angle, key_rgb=r.key_rgb)
        want = orc.render_stereo(op, d[k], c[k], want_depth=True, want_seed=seed)
        _compare({key: got[key][k] for key in ("sbs", "mask", "depth")}, want, W, f"{variant} 1080p frame {k}")
        if seed:
            for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                assert np.array_equal(got["seed"][k][:, sl].cpu().numpy(), want[eye + "_seed"]), f"{variant} seed {eye} frame {k}"
    r.close()


@pytest.mark.parametrize("W,H,fov", [(64, 48, 100), (33, 17, 120.5), (250, 61, 75), (640, 480, 90), (1920, 1920, 75)])
def test_equirect_remap_matches_the_oracle(mods, orc, W, H, fov):
    """convert_to_equirectangular (sr:25-86) on the device vs the oracle's cv2.remap restatement fed with the
    reference's own float32 maps: bit-exact, batched and through strided side-by-side views."""
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(W * 7 + H)
    img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    img[0, :, : W // 2] = np.linspace(0, 255, W // 2, dtype=np.uint8)[None, :, None]      # smooth part: weights matter
    want = np.stack([orc.convert_to_equirectangular(img[k], fov) for k in range(2)])
    t = torch.from_numpy(img).cuda()
    assert np.array_equal(sr.convert_to_equirectangular(t, fov).cpu().numpy(), want)
    assert np.array_equal(sr.convert_to_equirectangular(t[1], fov).cpu().numpy(), want[1])
    # strided: the two images as the eyes of one side-by-side buffer, remapped in place of cv2.hconcat's inputs
    sbs = torch.cat([t[0], t[1]], dim=1).contiguous()                                       # [H, 2W, 3]
    out = torch.zeros_like(sbs)
    sr.convert_to_equirectangular(sbs[:, :W], fov, out=out[:, :W])
    sr.convert_to_equirectangular(sbs[:, W:], fov, out=out[:, W:])
    assert np.array_equal(out.cpu().numpy(), np.concatenate([want[0], want[1]], axis=1))
    valid = np.any(want[0] != 0, axis=-1)
    assert valid[H // 2, W // 2] and not valid[0, 0]                                        # centred, black padding


def test_equirect_remap_rejects_bad_arguments(mods):
    _lib, sr, synthetic = mods
    t = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        sr.convert_to_equirectangular(t, 180)
    with pytest.raises(AssertionError):
        sr.convert_to_equirectangular(t, 90, out=t)
    ctx = _lib.Context(0, 16, 16)
    tx = torch.zeros(16, device="cuda")
    rc = _lib.load().mdvt_equirect_remap(ctx.handle, t.data_ptr(), 16, 0, t.data_ptr() + 1, 48, 0, 1, tx.data_ptr(), tx.data_ptr(), None)
    assert rc == -1 and b"pitch" in _lib.load().mdvt_last_error(ctx.handle)


@pytest.mark.parametrize("mode", ["points", "mesh", "mesh_infill"])
def test_mixed_batch_keeps_each_frames_own_arithmetic(mods, orc, mode):
    """A batch mixing pure-shift frames with pose / convergence frames: every frame equals the oracle run on
    that frame alone (the pure-shift / general selection is per frame, never per batch), with hole counts."""
    _lib, sr, synthetic = mods
    W, H, N = 128, 72, 7
    d, c = synthetic.SyntheticScene(W, H, config_id=2, n_fg=5).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=(mode == "points"), infill_mask=(mode == "mesh_infill"))
    T = synthetic.synthetic_pose_track(N)
    kinds = ["pure", "conv", "pure", "pure", "pose", "conv", "pure"]
    recs = [r.frame_params(xfov=45.0, convergence_distance=3.0 if k == "conv" else None,
                           transformation=T[t] if k == "pose" else None) for t, k in enumerate(kinds)]
    got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), recs, want_depth=True, want_hole_counts=True)
    for t, k in enumerate(kinds):
        want = _oracle(orc, r, recs[t], d[t], c[t], T=T[t] if k == "pose" else None)
        one = {key: got[key][t] for key in ("sbs", "mask", "depth")}
        _compare(one, want, W, tag=f"{mode} frame {t} ({k})")
        hc = got["hole_counts"][t].cpu().numpy()
        assert hc[0] == np.count_nonzero(want["left_mask"]) and hc[1] == np.count_nonzero(want["right_mask"])
    r.close()


def test_masked_blur_matches_the_oracle(mods, orc, golden):
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(3)
    for W, H in ((56, 40), (250, 61), (641, 33)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[H // 4:H // 2, W // 5:W // 2] = 0; img[:, :3] = 0; img[H - 1] = 0; img[2, 2] = (0, 0, 1)
        assert np.array_equal(sr.masked_blur(torch.from_numpy(img).cuda()).cpu().numpy(), orc.masked_blur(img))
    g = golden("masked_blur")                              # the reference's own glue (stubbed cv2 calls): <= 1 LSB
    got = sr.masked_blur(torch.from_numpy(g["a_img"]).cuda()).cpu().numpy()
    assert np.abs(got.astype(int) - g["a_out"].astype(int)).max() <= 1


def _synthetic_seed(rng, W, H, key=(0, 255, 0)):
    seed = np.zeros((H, W, 3), np.uint8)
    for _ in range(5):                                      # holes: key colour, normal-coloured points along their edges
        x0, y0 = int(rng.integers(1, W - 12)), int(rng.integers(1, H - 12))
        w, h = int(rng.integers(4, max(5, W // 4))), int(rng.integers(4, max(5, H // 3)))
        seed[y0:y0 + h, x0:x0 + w] = key
        for _ in range(w + h):
            seed[y0 + int(rng.integers(0, h)) if y0 + h <= H else y0, min(W - 1, x0 + int(rng.integers(0, 2)))] = rng.integers(1, 255, 3)
    seed[:, 0] = np.where(np.all(seed[:, 0] == key, -1)[:, None], np.array([255, 127, 127], np.uint8), seed[:, 0])
    return np.clip(seed[:H, :W], 0, 255)


@pytest.mark.parametrize("W,H", [(96, 64), (250, 61)])
def test_finish_infill_mask_matches_the_oracle(mods, orc, W, H):
    """sr:803-808 on the device (level-synchronous Telea inpaint + masked blur) vs the oracle, bit for bit: batched,
    through strided side-by-side views, with a round limit (same pixels left unfilled) and with a black key."""
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(W + H)
    seeds = np.stack([_synthetic_seed(rng, W, H) for _ in range(3)])
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    t = torch.from_numpy(seeds).cuda()
    got, rem = r.finish_infill_mask(t, want_remaining=True)
    for k in range(3):
        want, wrem = orc.finish_infill_mask(seeds[k])
        assert np.array_equal(got[k].cpu().numpy(), want), k
        assert int(rem[k]) == wrem == 0
        assert not np.any(np.all(want == (0, 255, 0), -1))                              # no key colour survives
        assert not want[np.all(seeds[k] == 0, -1)].any()                                # black (no hole) stays black
    # side-by-side layout: the two eyes are column halves of one buffer
    sbs = torch.cat([t[0], t[1]], dim=1).contiguous()
    out = torch.zeros_like(sbs)
    r.finish_infill_mask(sbs[:, :W], out=out[:, :W]); r.finish_infill_mask(sbs[:, W:], out=out[:, W:])
    assert np.array_equal(out.cpu().numpy(), np.concatenate([orc.finish_infill_mask(seeds[0])[0], orc.finish_infill_mask(seeds[1])[0]], 1))
    # both eyes of several frames in one pass (mdvt_finish_infill_mask_stereo): 10 frames = 20 images > one 16-image pass
    many = torch.stack([sbs] * 10)
    many[3, :, :W] = t[2]
    got_sbs, rem_sbs = r.finish_infill_mask_sbs(many, want_remaining=True)
    assert tuple(rem_sbs.shape) == (2, 10) and int(rem_sbs.sum()) == 0
    assert np.array_equal(got_sbs[0].cpu().numpy(), out.cpu().numpy()) and np.array_equal(got_sbs[9].cpu().numpy(), out.cpu().numpy())
    assert np.array_equal(got_sbs[3, :, :W].cpu().numpy(), orc.finish_infill_mask(seeds[2])[0])
    assert np.array_equal(got_sbs[3, :, W:].cpu().numpy(), orc.finish_infill_mask(seeds[1])[0])
    # round limit: the front stops after 2 levels, the same key-coloured pixels stay unfilled on both sides
    got2, rem2 = r.finish_infill_mask(t[2], max_rounds=2, want_remaining=True)
    want2, wrem2 = orc.finish_infill_mask(seeds[2], max_rounds=2)
    assert np.array_equal(got2.cpu().numpy(), want2) and int(rem2[0]) == wrem2 and wrem2 > 0
    r.close()
    # black key (no --infill_mask): every black pixel is to be filled and keeps its value (sr:803-807 with bg (0,0,0))
    rb = sr.StereoRerenderer(W, H, remove_edges=True)
    sb = seeds[0].copy(); sb[np.all(sb == (0, 255, 0), -1)] = 0
    gb = rb.finish_infill_mask(torch.from_numpy(sb).cuda(), max_rounds=W + H).cpu().numpy()
    wb, wr = orc.finish_infill_mask(sb, key_rgb=(0, 0, 0), max_rounds=W + H)
    assert np.array_equal(gb, wb) and wr == 0
    rb.close()


def test_finish_infill_mask_without_host_wait(mods):
    """The asynchronous form (max_rounds < 0 at the C-ABI: every level up to the bound gets its launches, none waits for the level
    count): the bytes and the `remaining` counts of the waiting form -- with the default bound, with a tight one, and with one
    that is too small (the same pixels stay unfilled)."""
    _lib, sr, synthetic = mods
    W, H = 250, 61
    rng = np.random.default_rng(77)
    seeds = np.stack([_synthetic_seed(rng, W, H) for _ in range(4)])
    sbs = torch.from_numpy(np.concatenate([seeds[:2], seeds[2:]], axis=2)).cuda()      # [2, H, 2W, 3]
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    for bound in (0, 40, 3):
        want, wrem = r.finish_infill_mask_sbs(sbs, max_rounds=bound, want_remaining=True)
        got, grem = r.finish_infill_mask_sbs(sbs, max_rounds=bound, want_remaining=True, no_host_wait=True)
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), bound
        assert np.array_equal(grem.cpu().numpy(), wrem.cpu().numpy()), bound
        assert (int(wrem.sum()) > 0) == (bound == 3)
    r.close()


def test_finish_infill_mask_wide_and_tall_images(mods, orc):
    """Rows beyond 2048 pixels take the two-vector row pass of the distance transform, images taller than 1088 rows the
    column pass that does not keep its segment in registers: one image that needs both, and an odd width beside it."""
    _lib, sr, synthetic = mods
    for W, H in ((2056, 1100), (2050, 40)):
        rng = np.random.default_rng(W)
        seed = np.zeros((H, W, 3), np.uint8)
        for _ in range(12):
            x0, y0 = int(rng.integers(1, W - 70)), int(rng.integers(1, H - 30))
            w, h = int(rng.integers(4, 60)), int(rng.integers(4, 28))
            seed[y0:y0 + h, x0:x0 + w] = (0, 255, 0)
            seed[y0:y0 + h:3, x0] = rng.integers(1, 255, 3)
            seed[y0 + h - 1, x0:x0 + w:4] = rng.integers(1, 255, 3)
        seed[H - 9:, W - 40:] = (0, 255, 0); seed[H - 9:, W - 41] = (9, 200, 77)         # a hole in the last rows / columns
        r = sr.StereoRerenderer(W, H, infill_mask=True)
        got, rem = r.finish_infill_mask(torch.from_numpy(seed).cuda(), want_remaining=True)
        want, wrem = orc.finish_infill_mask(seed)
        assert np.array_equal(got.cpu().numpy(), want), (W, H)
        assert int(rem[0]) == wrem == 0
        r.close()


@pytest.mark.parametrize("blocks", ["1", "3"])
def test_finish_infill_mask_with_a_starved_grid(mods, orc, monkeypatch, blocks):
    """The level passes of the completion with 1 / 3 workgroups (MDVT_TELEA_BLOCKS, re-read per call): every workgroup then
    loops over many list entries and marks far more pixels per target level than its LDS stage holds, so the direct
    append path, the multi-iteration loops and appends racing between workgroups all run -- same bits as the oracle."""
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")          # the hooks below exist in the tuning build only (csrc/mdvt_internal.h)
    _lib, sr, synthetic = mods
    monkeypatch.setenv("MDVT_TELEA_BLOCKS", blocks)
    W, H = 320, 180
    rng = np.random.default_rng(77)
    seeds = np.stack([_synthetic_seed(rng, W, H) for _ in range(2)])
    seeds[1, 40:140, 60:260] = (0, 255, 0)                  # one hole 100 x 200: 50 levels, thousands of needed pixels per level
    seeds[1, 40:140:7, 60] = (200, 90, 30); seeds[1, 139, 61:260:5] = (10, 220, 140)
    r = sr.StereoRerenderer(W, H, infill_mask=True)
    got, rem = r.finish_infill_mask(torch.from_numpy(seeds).cuda(), want_remaining=True)
    for k in range(2):
        want, wrem = orc.finish_infill_mask(seeds[k])
        assert np.array_equal(got[k].cpu().numpy(), want), k
        assert int(rem[k]) == wrem == 0
    r.close()


@pytest.mark.parametrize("mode,conv", [("mesh", None), ("mesh", 2.5), ("points", None)])
def test_infill_mask_and_basic_infill_from_a_render(mods, orc, mode, conv):
    """The product-default chain on real seeds: render(--infill_mask) -> seed -> finished mask, and the
    --do_basic_infill variant (edge points feed the mask only, holes filled by marching along its normals)."""
    _lib, sr, synthetic = mods
    W, H = 250, 141
    d, c = _scene(synthetic, W, H, seed=21, n_fg=5)
    for basic in (False, True):
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=(mode == "points"), infill_mask=True,
                                do_basic_infill=basic)
        p = r.frame_params(xfov=45.0, convergence_distance=conv)
        res = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_seed=True)
        op = orc.make_params(W, H, _K(p), ipd_m=0.065, depth_scale=p.depth_scale, mode=orc.MODE_POINTS if mode == "points" else orc.MODE_MESH,
                             remove_edges=True, edge_points=2 if basic else 1, conv_angle=p.convergence_angle, key_rgb=(0, 255, 0))
        want = orc.render_stereo(op, d, c, want_seed=True)
        _compare({"sbs": res["sbs"], "mask": res["mask"]}, want, W, tag=f"{mode} basic={basic}")
        for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
            assert np.array_equal(res["seed"][:, sl].cpu().numpy(), want[eye + "_seed"])
            fin = r.finish_infill_mask(res["seed"][:, sl])
            wfin, wrem = orc.finish_infill_mask(want[eye + "_seed"])
            assert wrem == 0 and np.array_equal(fin.cpu().numpy(), wfin), (mode, basic, eye)
            hole = want[eye + "_mask"] > 0
            assert np.array_equal(np.any(wfin != 0, -1), hole)                 # consumers' test: mask != black <=> hole
            if basic:
                normals = (fin.to(torch.float32) / 255.0) * 2 - 1              # sr:810
                img = sr.infill_using_normals(res["sbs"][:, sl], res["mask"][:, sl] > 0, normals).cpu().numpy()
                wn = ((wfin.astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)
                wimg = orc.infill_using_normals(want[eye + "_rgb"], hole, wn)
                assert np.array_equal(img, wimg)
                assert (np.all(img == 0, -1) & hole).sum() < 0.5 * hole.sum()  # most of the hole area got colour
        r.close()


def test_edge_filter_on_sub_millimetre_depths(mods, orc):
    """Regression (found by the widened sweep): content a fraction of a millimetre from the camera makes |n||v| of the
    89-degree test comparable with the reference's +1e-15 guard term, which the division-free screening ignores --
    such triangles must take the exact formula.  Depth codes 0..3 at max_depth 5 with a 25-degree master fov."""
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(109)
    W, H = 64, 32
    for trial in range(6):
        depth_rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        depth_rgb[..., 0] = 0
        depth_rgb[..., 2] = rng.integers(0, 4 + 3 * trial, (H, W))
        color = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
        for mesh in (True, False):
            r = sr.StereoRerenderer(W, H, pupillary_distance=0 if trial % 2 == 0 else 65, max_depth=5, master_xfov=25.0,
                                    render_as_pointcloud=not mesh, infill_mask=True, dont_place_points_in_edges=(trial < 3))
            p = r.frame_params(xfov=45.0)
            zs = orc.decode_depth(depth_rgb, 5, p.depth_scale)
            tri, unused, _ = orc.edge_filter(zs, _K(p), mesh)
            gt, gu = r.edge_filter(torch.from_numpy(depth_rgb).cuda(), p)
            assert np.array_equal(gt.cpu().numpy(), tri) and np.array_equal(gu.cpu().numpy(), unused), (trial, mesh)
            got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_depth=True)
            _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"tiny depths trial {trial} mesh={mesh}")
            r.close()


def test_randomised_aux_sweep(mods, orc):
    """Seeded random sweep over the stand-alone entry points (codec, Touchly plane, equirect remap, masked blur,
    normal-marching infill, mark_lower_side, normal_infill) against the oracle; MDVT_SWEEP_SEED / MDVT_SWEEP_CASES widen it."""
    import os
    _lib, sr, synthetic = mods
    from metric_depth_video_toolbox_amd import depth_frames_helper as dfh, infill_common, basic_nomal_infill
    rng = np.random.default_rng(int(os.environ.get("MDVT_SWEEP_SEED", "20260928")))
    n_cases = int(os.environ.get("MDVT_SWEEP_CASES", "12"))
    sizes = [(2, 2), (5, 3), (17, 9), (33, 17), (64, 48), (100, 31), (130, 70), (257, 129)]
    for case in range(n_cases):
        W, H = sizes[int(rng.integers(len(sizes)))]
        tag = f"aux#{case} {W}x{H}"
        # codec both ways
        md = int(rng.choice([5, 20, 100, 655])); scale = float(rng.choice([1.0, 0.37, 1.3938468501173518]))
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        z = dfh.decode_rgb_depth_frame(torch.from_numpy(rgb).cuda(), md, True, depth_scale=scale)
        assert np.array_equal(z.cpu().numpy().view(np.uint32), orc.decode_depth(rgb, md, scale).view(np.uint32)), tag
        d = (rng.uniform(-2, md * 1.2, (H, W)) * rng.choice([1.0, 1e-3])).astype(np.float32)
        enc = dfh.encode_depth_frame(torch.from_numpy(d).cuda(), md, bgr=False).cpu().numpy()
        assert np.array_equal(enc, orc.encode_depth(d, md)), tag
        # Touchly plane
        tmax, tmin = float(rng.uniform(1, 20)), float(rng.uniform(0, 0.9))
        for zf in (False, True):
            d8 = np.rint(np.maximum(0, np.minimum(np.abs(d), tmax) - tmin) * (255 / (tmax - tmin))).astype(np.uint8)
            if zf:
                d8[d8 == 0] = 255
            got = sr.touchly_depth(torch.from_numpy(np.abs(d)).cuda(), tmax, tmin, zero_is_far=zf).cpu().numpy()
            assert np.array_equal(got, np.repeat((255 - d8)[..., None], 3, axis=-1)), tag
        # equirect remap
        fov = float(rng.uniform(1.0, 179.0))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(sr.convert_to_equirectangular(torch.from_numpy(img).cuda(), fov).cpu().numpy(),
                              orc.convert_to_equirectangular(img, fov)), tag + f" fov {fov}"
        # masked blur
        bl = img.copy(); bl[rng.uniform(size=(H, W)) < rng.uniform(0, 0.9)] = 0
        assert np.array_equal(sr.masked_blur(torch.from_numpy(bl).cuda()).cpu().numpy(), orc.masked_blur(bl)), tag
        # normal-marching infill and mark_lower_side
        hole = rng.uniform(size=(H, W)) < rng.uniform(0, 0.6)
        ang = rng.uniform(0, 2 * np.pi, (H, W)); mag = rng.uniform(0, 1, (H, W))
        nrm = np.stack([np.cos(ang) * mag, np.sin(ang) * mag, rng.uniform(-1, 1, (H, W))], -1).astype(np.float32)
        nrm[rng.uniform(size=(H, W)) < 0.05] = (0.0, 1.0, 0.0)
        steps = int(rng.choice([3, 40, 400]))
        got = sr.infill_using_normals(torch.from_numpy(img).cuda(), torch.from_numpy(hole).cuda(), torch.from_numpy(nrm).cuda(), steps)
        assert np.array_equal(got.cpu().numpy(), orc.infill_using_normals(img, hole, nrm, steps)), tag
        msk = img.copy(); msk[~hole] = 0
        steps = int(rng.choice([2, 8, 30]))
        got = infill_common.mark_lower_side(torch.from_numpy(msk).cuda(), steps)
        assert np.array_equal(got.cpu().numpy(), orc.mark_lower_side(msk, steps)), tag
        # normal_infill (basic_nomal_infill.py:87-119): a random noise mask (every pixel its own direction, zero channels at
        # random) and a mask of a few blobs with coherent directions
        for kind in range(2):
            nmask = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            if kind == 0:
                nmask[rng.uniform(size=(H, W)) < rng.uniform(0.2, 0.95)] = 0
                nmask[rng.uniform(size=(H, W)) < 0.05, int(rng.integers(3))] = 0
            else:
                yy, xx = np.mgrid[0:H, 0:W]
                keep = np.zeros((H, W), bool)
                for _ in range(3):
                    keep |= (xx - rng.uniform(0, W)) ** 2 + (yy - rng.uniform(0, H)) ** 2 < rng.uniform(1, max(2.0, max(W, H) / 3)) ** 2
                base = rng.integers(1, 256, 3)
                nmask = np.clip(base[None, None, :] + rng.integers(-6, 7, (H, W, 3)), 1, 255).astype(np.uint8)
                nmask[~keep] = 0
            nimg = img.copy(); nimg[rng.uniform(size=(H, W)) < 0.1] = 0
            got = basic_nomal_infill.normal_infill(torch.from_numpy(nimg).cuda(), torch.from_numpy(nmask).cuda()).cpu().numpy()
            assert np.array_equal(got, orc.normal_infill(nimg, nmask)), tag + f" normal_infill kind {kind}"


def test_swap_rb_is_cvtcolor_bgr_rgb(mods):
    """cv2.cvtColor(BGR2RGB / RGB2BGR) (sr:493, 505, 928, 941) = the channel flip img[..., ::-1], batched, strided, in place."""
    _lib, sr, synthetic = mods
    from metric_depth_video_toolbox_amd import depth_frames_helper as dfh
    rng = np.random.default_rng(2)
    for W, H in ((250, 37), (64, 48), (1920, 8)):
        img = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        t = torch.from_numpy(img).cuda()
        assert np.array_equal(dfh.swap_rb(t).cpu().numpy(), img[..., ::-1])
        assert np.array_equal(dfh.swap_rb(t[1]).cpu().numpy(), img[1][..., ::-1])
        half = t[:, :, : W // 2]                                   # strided rows
        assert np.array_equal(dfh.swap_rb(half).cpu().numpy(), img[:, :, : W // 2, ::-1])
        dfh.swap_rb(t, out=t)                                       # in place
        assert np.array_equal(t.cpu().numpy(), img[..., ::-1])


@pytest.mark.parametrize("W", [10236, 10240, 6824, 6828, 4296, 4300, 5120])
def test_widths_around_the_lds_limits(mods, orc, W):
    """The last widths whose rows fit the LDS z-buffers and the first that do not (points 10 240 / 6 826 with edge points,
    mesh 5 120 / ~4 300): both sides of every switch-over render, and render the same thing."""
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(W)
    H = 3
    for mesh in (False, True):
        for infill in (False, True):
            d = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            d[..., 0] = rng.integers(2, 40, (H, W))
            c = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
            r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=not mesh, infill_mask=infill)
            p = r.frame_params(xfov=60.0)
            got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_depth=True)
            _compare(got, _oracle(orc, r, p, d, c), W, f"W={W} mesh={mesh} infill={infill}")
            r.close()


def _gl_fixture_names():
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import gl_parity
    return gl_parity.fixture_names()


@pytest.mark.parametrize("name", _gl_fixture_names())
def test_hip_against_gl_renders(mods, orc, name):
    """The HIP path against a conformant OpenGL's renders of the reference's own geometry (tests/golden/render_gl_*.npz,
    SwiftShader ES 3.0 through the view set-up of dmt.render, dmt:1422-1572; tests/golden/gen_gl_golden.py): rendered with
    mdvt_config.subpixel_bits = 4, the GL's grid, with and without back-face culling, and held to the GL by the rules of
    tests/gl_parity.py (hole mask and points bit for bit up to snap flips and depth pairs the GL's depth buffer cannot order;
    mesh colours within 1 LSB except on steep rubber-sheet triangles).  The oracle only supplies the plane of pixels the
    GL's depth resolution leaves open."""
    import gl_parity
    _lib, sr, synthetic = mods
    sc, g, T = gl_parity.load_fixture(name)
    W, points = sc["W"], bool(sc["pointcloud"])
    d, c = torch.from_numpy(g["depth_rgb"]).cuda(), torch.from_numpy(g["color_rgb"]).cuda()
    for cull in (False, True):
        r = sr.StereoRerenderer(W, sc["H"], pupillary_distance=sc["ipd_mm"], render_as_pointcloud=points, infill_mask=sc["remove_edges"],
                                dont_place_points_in_edges=True, cull=1 if cull else 0, subpixel_bits=4)
        p = r.frame_params(xfov=sc["xfov"], convergence_distance=sc["convergence"], transformation=T)
        got = r.render(d, c, p)
        sbs, mask = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy()
        op = gl_parity.oracle_params(orc, sc, T, cull, subpixel_bits=4)
        amb = orc.render_stereo_gl(op, g["depth_rgb"], g["color_rgb"], depth_tie_tol=orc.GL_DEPTH_TIE_TOL)
        for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
            tag = f"{eye}_c{int(cull)}s0"
            res = gl_parity.compare(sbs[:, sl], mask[:, sl], g[tag + "_rgb"], g[tag + "_mask"], amb[eye + "_ambiguous"], points)
            if sc["zero_patch"] and not points:      # GL clips at the near plane, the decree drops the triangle
                assert res["mask_diff"] <= 40, (name, tag, res)
                continue
            assert res["ok"], (name, tag, res)
            if not points and not sc["band"]:
                assert res["rgb_over_frac"] <= 0.01, (name, tag, res)
        r.close()


def test_hip_against_reference_renders(mods):
    """The HIP path against renders of the LITERAL reference (dmt.render through Open3D's own window), should
    tests/golden/gen_render_golden.py ever be run where the reference runs and its render_*.npz files be committed:
    BASELINE.json's bar -- hole mask bit-exact, RGB within 1 LSB.  The stage itself is pinned against a conformant GL
    (test_hip_against_gl_renders); what only such a render can settle is which GL states Open3D's window has
    (multisampling, culling, sub-pixel bits: profiles/r06_gl_parity.md)."""
    import glob, os, sys
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "golden", "render_[!g]*.npz")))
    if not files:
        pytest.skip("no render of the literal reference (Open3D window) committed: the rasteriser is pinned against a conformant "
                    "OpenGL instead (test_hip_against_gl_renders); the GL states of Open3D's window stay unobserved")
    _lib, sr, synthetic = mods
    sys.path.insert(0, os.path.join(here, "golden"))
    from render_scenes import RENDER_SCENES
    by_name = {s["name"]: s for s in RENDER_SCENES}
    for f in files:
        g = np.load(f, allow_pickle=False)
        sc = by_name[os.path.basename(f)[len("render_"):-len(".npz")]]
        T = None if g["T"].size == 0 else g["T"]
        r = sr.StereoRerenderer(sc["W"], sc["H"], pupillary_distance=sc["ipd_mm"], render_as_pointcloud=sc["pointcloud"],
                                infill_mask=sc["remove_edges"], dont_place_points_in_edges=True)
        p = r.frame_params(xfov=sc["xfov"], convergence_distance=sc["convergence"], transformation=T)
        got = r.render(torch.from_numpy(g["depth_rgb"]).cuda(), torch.from_numpy(g["color_rgb"]).cuda(), p)
        sbs, mask = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy()
        W = sc["W"]
        for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
            assert np.array_equal(mask[:, sl], g[eye + "_mask"]), f"{f} {eye}: hole mask differs from the reference render"
            keep = g[eye + "_mask"] == 0
            d = np.abs(sbs[:, sl].astype(int) - g[eye + "_rgb"].astype(int))[keep]
            assert d.max(initial=0) <= 1, f"{f} {eye}: RGB differs by up to {d.max()} LSB from the reference render"
        r.close()


def test_general_mesh_workspace_follows_the_budget_and_the_chunk_submitted(mods):
    """The posed / converged mesh path owns ~125 B per pixel and frame in flight (z keys, vertex records, colour side buffer,
    triangle queue, edge keys).  It is sized by what is submitted -- one frame: one slot -- and by mdvt_config.workspace_mib:
    with a 1 GiB budget a 16-frame 1080p batch of the product default stays under 1 GiB (4 frames per launch set instead of
    16) and renders the same bytes as with the default budget (16 slots, 4 GB)."""
    _lib, sr, synthetic = mods
    W, H, N = 1920, 1080, 16
    d, c = synthetic.SyntheticScene(W, H, config_id=2).clip(N)
    d, c = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    outs, sizes = [], []
    for mib in (1024, 0):
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True, workspace_mib=mib)
        ps = [r.frame_params(xfov=45.0, convergence_distance=2.5) for _ in range(N)]
        r.render(d[:1], c[:1], ps[:1])
        torch.cuda.synchronize()
        one = r.ctx.workspace_bytes()
        assert one < 300 << 20, f"a single 1080p frame allocated {one >> 20} MiB"
        got = r.render(d, c, ps, want_seed=True)
        torch.cuda.synchronize()
        sizes.append(r.ctx.workspace_bytes())
        outs.append({k: v.clone() for k, v in got.items()})
        r.close()
    assert sizes[0] <= (1024 << 20) + (8 << 20), f"{sizes[0] >> 20} MiB with a 1 GiB budget"
    assert sizes[1] > 3 * sizes[0]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_contexts_on_two_gpus_do_not_share_parameter_blocks(mods, orc):
    """the process-wide pool of pinned + device parameter blocks hands a block back only to a context on the GPU its
    device half was allocated on.  create / render / destroy on GPU 0, then create / render on GPU 1, then GPU 0 again."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _lib, sr, synthetic = mods
    W, H = 96, 64
    depth_rgb, color = _scene(synthetic, W, H, seed=7)
    for dev in (0, 1, 0, 1):
        with torch.cuda.device(dev):
            r = sr.StereoRerenderer(W, H, device=dev, pupillary_distance=65)
            p = r.frame_params(xfov=45.0)
            got = r.render(torch.from_numpy(depth_rgb).cuda(dev), torch.from_numpy(color).cuda(dev), p, want_depth=True)
            _compare(got, _oracle(orc, r, p, depth_rgb, color), W, f"device {dev}")
            r.close()


def test_finish_infill_mask_in_two_concurrent_halves(mods):
    """finish_infill_mask_sbs splits a call of FINISH_SPLIT_FRAMES frames or more into two halves on two contexts and two streams
    (the marking pass of the completion waits most of its cycles; a second pass beside it fills them).  A frame's finished mask
    does not depend on its batch: the split call gives the bytes of the unsplit one, and the same counts of unreached pixels."""
    _lib, sr, synthetic = mods
    W, H, N = 320, 180, 8
    d, c = synthetic.SyntheticScene(W, H, config_id=3, n_fg=8).clip(N)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, infill_mask=True)
    ps = [r.frame_params(xfov=45.0, convergence_distance=2.5 if k % 2 else None) for k in range(N)]
    seed = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), ps, want_seed=True)["seed"]
    whole, rem_w = r.finish_infill_mask_sbs(seed, want_remaining=True, max_rounds=20)
    r.FINISH_SPLIT_FRAMES = 4                      # (instance attribute: this renderer only)
    for _ in range(2):                             # second time: the second context and its workspace exist
        halves, rem_h = r.finish_infill_mask_sbs(seed, want_remaining=True, max_rounds=20)
        torch.cuda.synchronize()
        assert torch.equal(whole, halves) and torch.equal(rem_w, rem_h)
    assert int(rem_w.sum()) > 0, "max_rounds = 20 should leave deep holes unreached in some frame (the counts are being compared)"
    r.close()
