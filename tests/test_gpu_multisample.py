"""The opt-in 4x multisampled render (StereoRerenderer(samples=4), mdvt_config.samples, csrc/mdvt_msaa.hip) against the oracle's
multisample candidate orc_render_stereo_gl(samples=4, pattern, resolve), bit for bit, and against the conformant GL's own 4x
multisampled renders (tests/golden/render_gl_*.npz, keys *s4_*).  The oracle's parameters are built from the renderer's own
sub-pixel grid, so MDVT_TEST_SUBPIXEL_BITS=4 runs this file on the 4-bit copy of the kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MDVT_ERR_INVALID_ARG = -1
MDVT_ERR_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, synthetic
    return _lib, stereo_rerender, synthetic


def _K(p):
    return np.array([p.K[k] for k in range(9)]).reshape(3, 3)


def _oracle_ms(orc, r, p, depth_rgb, color, T=None):
    op = orc.make_params(r.W, r.H, _K(p), ipd_m=r.pupillary_distance / 1000, max_depth=r.max_depth, depth_scale=p.depth_scale,
                         mode=orc.MODE_POINTS if r.mode == 0 else orc.MODE_MESH, remove_edges=r.remove_edges, edge_points=False,
                         conv_angle=p.convergence_angle, T=T, key_rgb=r.key_rgb, cull=r.cull, subpixel_bits=r.subpixel_bits)
    return orc.render_stereo_gl(op, depth_rgb, color, samples=4, pattern=r.sample_pattern, resolve=r.sample_resolve)


def _compare(got, want, W, tag=""):
    sbs, mask = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy()
    for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
        m, wm = mask[:, sl], want[eye + "_mask"]
        assert np.array_equal(m, wm), f"{tag} {eye} mask differs at {int((m != wm).sum())} px"
        c, wc = sbs[:, sl], want[eye + "_rgb"]
        assert np.array_equal(c, wc), f"{tag} {eye} rgb differs at {int(np.any(c != wc, axis=-1).sum())} px"


# (the scene styles of test_gpu_render.py, copied: key-coloured pixels, depth-code-0 patches, one-LSB depths)
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


def _stripes(W, H, near=120, far=30000, period=2, rows=False):
    """Alternating near / far columns (or rows): maximal folding, the rubber sheet everywhere."""
    idx = (np.arange(H)[:, None] if rows else np.arange(W)[None, :]) // period % 2
    code = np.where(np.broadcast_to(idx, (H, W)) == 0, near, far).astype(np.uint32)
    d = np.zeros((H, W, 3), np.uint8)
    d[..., 0] = (code >> 8) & 0xFF
    d[..., 2] = code & 0xFF
    return d


def _ties_scene(synthetic, W, H, t=180):
    """C4's contention band: hundreds of cells folded onto a few pixels, exact depth ties between colours."""
    from metric_depth_video_toolbox_amd.depth_map_tools import compute_camera_matrix
    K = compute_camera_matrix(45.0, None, W, H)
    sc = synthetic.SyntheticScene(W, H, config_id=4)
    z = synthetic.contention_band(sc.depth_m(t), K[0, 0], 0.065, row0=H // 3, rows=H // 3)
    _, color = sc.frame(t)
    return synthetic.quantise_depth_to_rgb(z), color


def _frame(r, synthetic, kind, xfov=45.0):
    T = synthetic.synthetic_pose_track(40)[37] if kind in ("pose", "both") else None
    conv = 2.5 if kind in ("convergence", "both") else None
    return r.frame_params(xfov=xfov, convergence_distance=conv, transformation=T), T


def _render_and_check(mods, orc, depth_rgb, color, kind, tag, **kw):
    _lib, sr, synthetic = mods
    H, W = depth_rgb.shape[:2]
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, samples=4, **kw)
    p, T = _frame(r, synthetic, kind)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_hole_counts=True)
    _compare(got, _oracle_ms(orc, r, p, depth_rgb, color, T), W, f"{tag} {kind} {W}x{H} {kw}")
    mask, counts = got["mask"].cpu().numpy(), got["hole_counts"].cpu().numpy()
    assert int(counts[0]) == int(mask[:, :W].sum()) // 255 and int(counts[1]) == int(mask[:, W:].sum()) // 255, f"{tag} hole counts"
    r.close()


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the oracle
KINDS = ["pure", "convergence", "pose", "both"]


@pytest.mark.parametrize("cull", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_multisample_matches_oracle(mods, orc, mode, kind, cull):
    _lib, sr, synthetic = mods
    combos = [(0, 0), (1, 1), (0, 1), (1, 0)]
    for n, (W, H) in enumerate([(33, 17), (96, 64), (250, 37)]):
        depth_rgb, color = _scene(synthetic, W, H, seed=7 + n)
        P, R = combos[(n + cull) % 4]
        flags = [dict(), dict(remove_edges=True, dont_place_points_in_edges=True),
                 dict(infill_mask=True, dont_place_points_in_edges=True)][n]
        _render_and_check(mods, orc, depth_rgb, color, kind, "scene", render_as_pointcloud=mode == "points", cull=cull,
                          sample_pattern=P, sample_resolve=R, **flags)


@pytest.mark.parametrize("P,R", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_multisample_patterns_and_resolves_640x480(mods, orc, mode, P, R):
    _lib, sr, synthetic = mods
    depth_rgb, color = _scene(synthetic, 640, 480, seed=12)
    for kind in ("pure", "both"):
        _render_and_check(mods, orc, depth_rgb, color, kind, "640x480", render_as_pointcloud=mode == "points",
                          sample_pattern=P, sample_resolve=R, infill_mask=True, dont_place_points_in_edges=True)


@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_multisample_hard_scenes(mods, orc, mode):
    """Near / far stripes (the rubber sheet: large triangles across depth edges) and exact depth ties between colours."""
    _lib, sr, synthetic = mods
    pts = mode == "points"
    for W, H, rows in ((96, 40, False), (64, 48, True)):
        d = _stripes(W, H, rows=rows)
        color = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        for kind in KINDS:
            _render_and_check(mods, orc, d, color, kind, "stripes", render_as_pointcloud=pts, sample_pattern=1, sample_resolve=1)
    d, color = _ties_scene(synthetic, 256, 96)
    for cull in (0, 2):
        _render_and_check(mods, orc, d, color, "pure", "ties", render_as_pointcloud=pts, cull=cull)
    _render_and_check(mods, orc, d, color, "pure", "ties+edges", render_as_pointcloud=pts, remove_edges=True,
                      dont_place_points_in_edges=True, sample_pattern=1)


@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_multisample_full_hd_and_wide_frames(mods, orc, mode):
    """One 1920 x 1080 frame, and a frame wider than the LDS row kernels take (5000 px)."""
    _lib, sr, synthetic = mods
    pts = mode == "points"
    depth_rgb, color = _scene(synthetic, 1920, 1080, seed=5)
    _render_and_check(mods, orc, depth_rgb, color, "pure", "1080p", render_as_pointcloud=pts)
    _render_and_check(mods, orc, depth_rgb, color, "pose", "1080p", render_as_pointcloud=pts, sample_pattern=1, sample_resolve=1,
                      remove_edges=True, dont_place_points_in_edges=True)
    depth_rgb, color = _scene(synthetic, 5000, 24, seed=6)
    for kind in ("pure", "both"):
        _render_and_check(mods, orc, depth_rgb, color, kind, "wide", render_as_pointcloud=pts, cull=1 if not pts else 0)


# ------------------------------------------------------------------------------------------------ 2. batches and layouts
@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_multisample_batch_with_padded_pitches(mods, orc, mode):
    """9 frames in one call -- pure-shift and posed frames mixed, a field of view per frame, padded rows and separate eye buffers,
    a workspace budget of 2 frames in flight -- equal frame-by-frame oracle renders; hole counts equal the masks."""
    _lib, sr, synthetic = mods
    W, H, N = 120, 66, 9
    pad_in, pad_out, pad_m = 21, 15, 5
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=mode == "points", samples=4, sample_pattern=1,
                            infill_mask=True, dont_place_points_in_edges=True, workspace_mib=1)
    poses = synthetic.synthetic_pose_track(N)
    scenes = [_scene(synthetic, W, H, seed=40 + f) for f in range(N)]
    params, Ts = [], []
    for f in range(N):
        T = poses[f] if f % 3 == 1 else None
        params.append(r.frame_params(xfov=40.0 + 3 * f, convergence_distance=3.0 if f % 3 == 2 else None, transformation=T))
        Ts.append(T)
    ip, op, mp = 3 * W + pad_in, 3 * W + pad_out, W + pad_m
    dbuf = torch.zeros((N, H, ip), dtype=torch.uint8, device="cuda")
    cbuf = torch.zeros((N, H, ip), dtype=torch.uint8, device="cuda")
    for f, (d, c) in enumerate(scenes):
        dbuf[f, :, :3 * W] = torch.from_numpy(d.reshape(H, 3 * W)).cuda()
        cbuf[f, :, :3 * W] = torch.from_numpy(c.reshape(H, 3 * W)).cuda()
    outs = {k: torch.full((N, H, op), 7, dtype=torch.uint8, device="cuda") for k in "lr"}
    masks = {k: torch.full((N, H, mp), 7, dtype=torch.uint8, device="cuda") for k in "lr"}
    counts = torch.full((N, 2), 12345, dtype=torch.int32, device="cuda")
    io = _lib.MdvtIO()
    io.depth_rgb, io.depth_pitch, io.depth_stride = dbuf.data_ptr(), ip, ip * H
    io.color_rgb, io.color_pitch, io.color_stride = cbuf.data_ptr(), ip, ip * H
    io.left_rgb, io.right_rgb, io.rgb_pitch, io.rgb_stride = outs["l"].data_ptr(), outs["r"].data_ptr(), op, op * H
    io.left_mask, io.right_mask, io.mask_pitch, io.mask_stride = masks["l"].data_ptr(), masks["r"].data_ptr(), mp, mp * H
    io.hole_counts = counts.data_ptr()
    arr = sr.StereoRerenderer.pack_params(params, N)
    s = torch.cuda.current_stream()
    r.ctx.check(_lib.load().mdvt_render_stereo_batch(r.ctx.handle, N, arr, C.byref(io), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    assert r.ctx.workspace_bytes() >= 64 * W * H, "the sample key planes are reported as workspace"
    cnt = counts.cpu().numpy()
    for f in range(N):
        want = _oracle_ms(orc, r, params[f], scenes[f][0], scenes[f][1], Ts[f])
        for eye, k in ((0, "l"), (1, "r")):
            name = ("left", "right")[eye]
            rgb = outs[k][f, :, :3 * W].cpu().numpy().reshape(H, W, 3)
            m = masks[k][f, :, :W].cpu().numpy()
            assert np.array_equal(rgb, want[name + "_rgb"]) and np.array_equal(m, want[name + "_mask"]), (mode, f, name)
            assert (outs[k][f, :, 3 * W:] == 7).all() and (masks[k][f, :, W:] == 7).all(), "padding must stay untouched"
            assert int(cnt[f, eye]) == int(m.sum()) // 255, (mode, f, name, "hole count")
    r.close()


# ------------------------------------------------------------------------------------------------ 3. the conformant GL's 4x renders
def _gl_names():
    import gl_parity
    return gl_parity.fixture_names()


@pytest.mark.parametrize("name", _gl_names())
def test_multisample_against_gl_renders(mods, orc, name):
    """Every render_gl_* scene on the GL's grid (4 bits) with its sample pattern and resolve (SwiftShader: 1, 1), with and without
    back-face culling: the HIP render equals the oracle's candidate and meets the rule test_oracle_golden.py holds the candidate to
    against the GL's own 4x multisampled renders (the mesh scenes with Z = 0 patches are left out there, and here)."""
    import gl_parity
    _lib, sr, synthetic = mods
    sc, g, T = gl_parity.load_fixture(name)
    W, H, points = sc["W"], sc["H"], bool(sc["pointcloud"])
    for cull in (False, True):
        r = sr.StereoRerenderer(W, H, pupillary_distance=sc["ipd_mm"], render_as_pointcloud=points, remove_edges=sc["remove_edges"],
                                infill_mask=sc["remove_edges"], dont_place_points_in_edges=True, cull=1 if cull else 0,
                                subpixel_bits=4, samples=4, sample_pattern=1, sample_resolve=1)
        p = r.frame_params(xfov=sc["xfov"], convergence_distance=sc["convergence"], transformation=T)
        got = r.render(torch.from_numpy(np.ascontiguousarray(g["depth_rgb"])).cuda(), torch.from_numpy(np.ascontiguousarray(g["color_rgb"])).cuda(), p)
        r.close()
        op = gl_parity.oracle_params(orc, sc, T, cull, subpixel_bits=4)
        ms = orc.render_stereo_gl(op, g["depth_rgb"], g["color_rgb"], samples=4, pattern=1, resolve=1, depth_tie_tol=orc.GL_DEPTH_TIE_TOL)
        _compare(got, ms, W, f"{name} cull={cull}")
        if sc["zero_patch"] and not points:
            continue
        sbs, mask = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy()
        for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
            tag = f"{eye}_c{int(cull)}"
            r4 = gl_parity.compare(sbs[:, sl], mask[:, sl], g[tag + "s4_rgb"], g[tag + "s4_mask"], ms[eye + "_ambiguous"], False)
            assert r4["mask_diff"] <= r4["allowed"] and r4["unexplained"] <= 4 * r4["allowed"], (name, tag + "s4", r4)


# ------------------------------------------------------------------------------------------------ 4. off means off
@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_single_sample_settings_change_nothing(mods, mode):
    _lib, sr, synthetic = mods
    W, H = 160, 90
    depth_rgb, color = _scene(synthetic, W, H, seed=3)
    d, c = torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda()
    base = dict(pupillary_distance=65, render_as_pointcloud=mode == "points", infill_mask=True)
    for kind in ("pure", "pose"):
        outs = []
        for kw in (dict(), dict(samples=0), dict(samples=1)):
            r = sr.StereoRerenderer(W, H, **base, **kw)
            p, _ = _frame(r, synthetic, kind)
            got = r.render(d, c, p, want_depth=True, want_seed=True, want_maskbits=True, want_hole_counts=True)
            outs.append({k: v.cpu().numpy() for k, v in got.items()})
            r.close()
        for o in outs[1:]:
            for k in outs[0]:
                assert np.array_equal(o[k], outs[0][k]), (mode, kind, k)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_multisample_refusals(mods):
    _lib, sr, synthetic = mods
    W, H = 64, 48
    L = _lib.load()
    ctx = _lib.Context(torch.cuda.current_device(), W, H)
    for field, value, word in (("samples", 2, "samples"), ("samples", 8, "samples"), ("samples", -1, "samples"),
                               ("sample_pattern", 2, "sample_pattern"), ("sample_resolve", 2, "sample_resolve")):
        cfg = _lib.MdvtConfig()
        cfg.mode, cfg.max_depth, cfg.ipd_m = 1, 100.0, 0.065
        setattr(cfg, field, value)
        rc = L.mdvt_set_config(ctx.handle, C.byref(cfg))
        assert rc == MDVT_ERR_INVALID_ARG and word in L.mdvt_last_error(ctx.handle).decode(), (field, value)
        with pytest.raises(ValueError, match=word):
            kw = dict(samples=4)
            kw[field] = value
            sr.StereoRerenderer(W, H, **kw)
    ctx.close()
    depth_rgb, color = _scene(synthetic, W, H, seed=1)
    d, c = torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda()
    r = sr.StereoRerenderer(W, H, samples=4, infill_mask=True)                 # edge points on (sr:589)
    with pytest.raises(_lib.MdvtError, match="edge points") as e:
        r.render(d, c, r.frame_params(xfov=45.0))
    assert e.value.code == MDVT_ERR_UNSUPPORTED
    r.close()
    r = sr.StereoRerenderer(W, H, samples=4, infill_mask=True, dont_place_points_in_edges=True)
    p = r.frame_params(xfov=45.0)
    for kw, word in ((dict(want_depth=True), "depth planes"), (dict(want_seed=True), "seed images"),
                     (dict(want_maskbits=True), "packed mask bits"), (dict(want_maskbits=True, want_mask=False), "packed mask bits")):
        with pytest.raises(_lib.MdvtError, match=word) as e:
            r.render(d, c, p, **kw)
        assert e.value.code == MDVT_ERR_UNSUPPORTED, kw
    r.render(d, c, p, want_hole_counts=True)                                    # ... and the context still renders
    r.close()


# ------------------------------------------------------------------------------------------------ 6. randomised sweep
def ms_sweep_cases(synthetic):
    """MDVT_MS_SWEEP_SEED / MDVT_MS_SWEEP_CASES widen the sweep (soaks) without touching the default."""
    rng = np.random.default_rng(int(os.environ.get("MDVT_MS_SWEEP_SEED", "20261015")))
    sizes = [(2, 2), (3, 2), (5, 3), (8, 8), (17, 9), (36, 20), (61, 33), (100, 31), (128, 16), (200, 12)]
    for case in range(int(os.environ.get("MDVT_MS_SWEEP_CASES", "40"))):
        W, H = sizes[int(rng.integers(len(sizes)))]
        depth_rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        style = int(rng.integers(5))
        if style == 0:                                   # smooth plane + a step
            code = (2000 + 40 * np.arange(W)[None, :] + 7 * np.arange(H)[:, None]).astype(np.uint32)
            code[:, W // 2:] //= 3
            depth_rgb[..., 0], depth_rgb[..., 2] = (code >> 8) & 0xFF, code & 0xFF
        elif style == 1:                                 # very near content: huge disparities, near-plane rejects
            depth_rgb[..., 0] = 0
            depth_rgb[..., 2] = rng.integers(0, 4, (H, W))
        elif style == 2:                                 # constant depth: exact ties everywhere
            depth_rgb[..., 0], depth_rgb[..., 2] = 3, 77
        elif style == 3:                                 # near / far stripes
            depth_rgb = _stripes(W, H, near=int(rng.integers(20, 400)), far=int(rng.integers(5000, 65000)),
                                 period=int(rng.integers(1, 4)), rows=bool(rng.integers(2)))
        color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        kw = dict(pupillary_distance=int(rng.choice([0, 30, 63, 120, 400])), max_depth=int(rng.choice([5, 20, 100, 655])),
                  master_xfov=float(rng.choice([25.0, 45.0, 70.0])), render_as_pointcloud=bool(rng.integers(2)),
                  cull=int(rng.integers(3)), sample_pattern=int(rng.integers(2)), sample_resolve=int(rng.integers(2)))
        if rng.integers(2):
            kw.update(infill_mask=True, dont_place_points_in_edges=True)
        if rng.integers(2):
            color[rng.integers(H), rng.integers(W)] = (0, 255, 0) if kw.get("infill_mask") else (0, 0, 0)
        yield dict(case=case, depth_rgb=depth_rgb, color=color, kind=KINDS[int(rng.integers(4))],
                   xfov=float(rng.choice([20.0, 45.0, 90.0, 120.0])), kw=kw, style=style)


def test_multisample_randomised_sweep(mods, orc):
    _lib, sr, synthetic = mods
    for cs in ms_sweep_cases(synthetic):
        d, c = cs["depth_rgb"], cs["color"]
        H, W = d.shape[:2]
        r = sr.StereoRerenderer(W, H, samples=4, **cs["kw"])
        p, T = _frame(r, synthetic, cs["kind"], xfov=cs["xfov"])
        got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_hole_counts=True)
        tag = f"ms-sweep#{cs['case']} {W}x{H} {cs['kind']} style={cs['style']} {cs['kw']}"
        _compare(got, _oracle_ms(orc, r, p, d, c, T), W, tag)
        m, cnt = got["mask"].cpu().numpy(), got["hole_counts"].cpu().numpy()
        assert int(cnt[0]) == int(m[:, :W].sum()) // 255 and int(cnt[1]) == int(m[:, W:].sum()) // 255, tag + " counts"
        r.close()


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_cli_multisample_end_to_end(mods, tmp_path):
    _lib, sr, synthetic = mods
    W, H, N = 96, 54, 3
    scene = synthetic.SyntheticScene(W, H, seed=8, n_fg=5)
    depth, color = scene.clip(N)
    dp, cp = str(tmp_path / "d.npy"), str(tmp_path / "c.npy")
    np.save(dp, depth)
    np.save(cp, color)
    rc = sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "50", "--pupillary_distance", "65", "--batch", "2",
                  "--multisample", "4", "--sample_pattern", "swiftshader", "--render_as_pointcloud"])
    assert rc == 0
    sbs, mask = np.load(dp + "_stereo.npy"), np.load(dp + "_stereo.npy_holemask.npy")
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, render_as_pointcloud=True, samples=4, sample_pattern=1, sample_resolve=1)
    p = r.frame_params(xfov=50.0)
    got = r.render(torch.from_numpy(np.ascontiguousarray(depth)).cuda(), torch.from_numpy(np.ascontiguousarray(color)).cuda(), [p] * N)
    assert np.array_equal(sbs, got["sbs"].cpu().numpy())
    assert np.array_equal(mask.reshape(N, H, 2 * W), got["mask"].cpu().numpy())
    r.close()
    os.remove(dp + "_stereo.npy")
    with pytest.raises(ValueError, match="dont_place_points_in_edges"):
        sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "50", "--multisample", "4", "--infill_mask"])
    assert not os.path.exists(dp + "_stereo.npy")
