"""Opt-in near-plane clipping of the mesh (StereoRerenderer(near_clip=True), mdvt_set_near_clip, csrc/mdvt_near_clip.hip) against the
oracle's candidate orc_render_stereo_gl(near_clip=1, samples, pattern, resolve), bit for bit, both eyes, RGB, mask and hole counts;
against the conformant GL's renders of the Z = 0 patch fixture; and byte-identical to the default render wherever nothing
crosses the near plane."""
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


def _oracle(orc, r, p, depth_rgb, color, T=None):
    op = orc.make_params(r.W, r.H, _K(p), ipd_m=r.pupillary_distance / 1000, max_depth=r.max_depth, depth_scale=p.depth_scale,
                         mode=orc.MODE_POINTS if r.mode == 0 else orc.MODE_MESH, remove_edges=r.remove_edges, edge_points=False,
                         conv_angle=p.convergence_angle, T=T, key_rgb=r.key_rgb, cull=r.cull, subpixel_bits=r.subpixel_bits)
    return orc.render_stereo_gl(op, depth_rgb, color, near_clip=True, samples=r.samples, pattern=r.sample_pattern,
                                resolve=r.sample_resolve)


def _compare(got, want, W, tag=""):
    sbs, mask = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy()
    for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
        m, wm = mask[:, sl], want[eye + "_mask"]
        assert np.array_equal(m, wm), f"{tag} {eye} mask differs at {int((m != wm).sum())} px"
        c, wc = sbs[:, sl], want[eye + "_rgb"]
        assert np.array_equal(c, wc), f"{tag} {eye} rgb differs at {int(np.any(c != wc, axis=-1).sum())} px"


def _tz(z):
    T = np.eye(4)
    T[2, 3] = z
    return T


def _scene(synthetic, W, H, seed, patch=True, config_id=None):
    """A synthetic frame with a depth-code-0 patch (Z = 0: behind the near plane) and exact key colours."""
    if config_id is None:
        depth_rgb, color = synthetic.SyntheticScene(W, H, seed=seed, n_fg=6).frame(0)
    else:
        depth_rgb, color = synthetic.SyntheticScene(W, H, config_id=config_id).frame(seed)
    if patch and H > 8 and W > 16:
        h, w = max(3, H // 10), max(6, W // 10)
        depth_rgb[H // 3:H // 3 + h, W // 4:W // 4 + w] = 0
        depth_rgb[3:5, W - 9:W - 4] = 0
        color[1, 2] = (0, 0, 0)
        color[2, 7] = (0, 255, 0)
    return depth_rgb, color


# frame kind -> (convergence distance, pose, Z = 0 patch, scene config of SyntheticScene or None)
def _kind(synthetic, kind):
    return {"pure": (None, None, True, None), "convergence": (2.5, None, True, None),
            "pose2": (None, _tz(-2.0), False, 2), "pose5": (None, _tz(-5.0), False, 2),
            "pose_patch": (None, synthetic.synthetic_pose_track(40)[37], True, None)}[kind]


KINDS = ["pure", "convergence", "pose2", "pose5", "pose_patch"]


def _check(mods, orc, W, H, kind, tag, seed=3, scene=None, **kw):
    _lib, sr, synthetic = mods
    conv, T, patch, cfg = _kind(synthetic, kind)
    depth_rgb, color = scene if scene is not None else _scene(synthetic, W, H, seed, patch=patch, config_id=cfg)
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, near_clip=True, **kw)
    p = r.frame_params(xfov=45.0, convergence_distance=conv, transformation=T)
    got = r.render(torch.from_numpy(depth_rgb).cuda(), torch.from_numpy(color).cuda(), p, want_hole_counts=True)
    want = _oracle(orc, r, p, depth_rgb, color, T)
    _compare(got, want, W, f"{tag} {kind} {W}x{H} {kw}")
    mask, counts = got["mask"].cpu().numpy(), got["hole_counts"].cpu().numpy()
    assert int(counts[0]) == int(mask[:, :W].sum()) // 255 and int(counts[1]) == int(mask[:, W:].sum()) // 255, f"{tag} hole counts"
    r.close()
    return want


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("samples", [1, 4])
def test_near_clip_matches_oracle(mods, orc, kind, samples):
    """Every frame kind with both sample counts, cull 0 / 1 / 2, edge removal, both grids and (4x) both patterns and resolves."""
    edges = dict(remove_edges=True, dont_place_points_in_edges=True)
    cases = [((33, 17), dict(cull=0)), ((96, 64), dict(cull=1, **edges)), ((121, 45), dict(cull=2, subpixel_bits=4)),
             ((160, 90), dict(cull=0, infill_mask=True, dont_place_points_in_edges=True, subpixel_bits=4))]
    for n, ((W, H), kw) in enumerate(cases):
        ms = dict(samples=4, sample_pattern=n % 2, sample_resolve=(n // 2) % 2) if samples == 4 else dict(samples=samples if n % 2 else 0)
        _check(mods, orc, W, H, kind, "case", seed=5 + n, **kw, **ms)


def test_near_clip_straddles_are_really_clipped(mods, orc):
    """The parity cases above are not vacuous: the oracle's clipped render differs from the decree's on these frames."""
    _lib, sr, synthetic = mods
    for kind in ("pure", "pose2"):
        conv, T, patch, cfg = _kind(synthetic, kind)
        d, c = _scene(synthetic, 96, 64, 6, patch=patch, config_id=cfg)
        r = sr.StereoRerenderer(96, 64, pupillary_distance=65)
        p = r.frame_params(xfov=45.0, transformation=T)
        got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p)
        want = _oracle(orc, r, p, d, c, T)
        sbs = got["sbs"].cpu().numpy()
        assert not (np.array_equal(sbs[:, :96], want["left_rgb"]) and np.array_equal(sbs[:, 96:], want["right_rgb"])), kind
        r.close()


@pytest.mark.parametrize("samples", [1, 4])
def test_near_clip_larger_frames(mods, orc, samples):
    """640 x 480 (pure shift and convergence with Z = 0 patches), 320 x 180 under the -2 m and -5 m poses of the issue's measurement,
    one posed 1920 x 1080 frame, and a frame wider than the LDS row kernels take (5000 px)."""
    ms = dict(samples=4, sample_pattern=1, sample_resolve=1) if samples == 4 else {}
    _check(mods, orc, 640, 480, "pure", "640x480", **ms)
    _check(mods, orc, 640, 480, "convergence", "640x480", cull=1, remove_edges=True, dont_place_points_in_edges=True, **ms)
    for kind in ("pose2", "pose5"):
        _check(mods, orc, 320, 180, kind, "320x180", **ms)
    if samples == 1:
        _lib, sr, synthetic = mods
        d, c = synthetic.SyntheticScene(1920, 1080, seed=3, n_fg=6).frame(0)
        d[500:506, 900:908] = 0                                   # (a small patch: the oracle walks every fan triangle's whole box)
        _check(mods, orc, 1920, 1080, "pose_patch", "1080p", scene=(d, c))
    _check(mods, orc, 5000, 24, "pure", "wide", cull=2, **ms)


def test_near_clip_degenerate_pose_equal_depths(mods, orc):
    """A pose that flattens every vertex to Z' = 1: a code-0 vertex (behind: zsrc = 0) and its neighbour have the same eye-space depth,
    tt = -inf and the new vertices lie at infinity (snap-clamped), colours +-inf / NaN.  The oracle's bytes."""
    _lib, sr, synthetic = mods
    T = np.diag([1.0, 1.0, 0.0, 1.0])
    T[2, 3] = 1.0
    for samples in (1, 4):
        W, H = 48, 30
        d, c = _scene(synthetic, W, H, 9)
        r = sr.StereoRerenderer(W, H, pupillary_distance=65, near_clip=True, samples=samples)
        p = r.frame_params(xfov=45.0, transformation=T)
        got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p)
        _compare(got, _oracle(orc, r, p, d, c, T), W, f"degenerate samples={samples}")
        r.close()


# ------------------------------------------------------------------------------------------------ 2. the conformant GL's renders
@pytest.mark.parametrize("cull", [False, True])
def test_near_clip_against_gl_zero_patch_fixture(mods, orc, cull):
    """render_gl_mesh_zero_patch_96x60 on the GL's grid: the left eye's mask equals the GL's exactly, single-sample and 4x (SwiftShader
    pattern and resolve); the right eye equals the candidate (this GL loses the polygon with w = 0 exactly and draws no streak)."""
    import gl_parity
    _lib, sr, synthetic = mods
    sc, g, T = gl_parity.load_fixture("mesh_zero_patch_96x60")
    W = sc["W"]
    d, c = np.ascontiguousarray(g["depth_rgb"]), np.ascontiguousarray(g["color_rgb"])
    for samples in (0, 4):
        r = sr.StereoRerenderer(W, sc["H"], pupillary_distance=sc["ipd_mm"], cull=1 if cull else 0, subpixel_bits=4, near_clip=True,
                                samples=samples, sample_pattern=1 if samples else 0, sample_resolve=1 if samples else 0)
        p = r.frame_params(xfov=sc["xfov"], convergence_distance=sc["convergence"], transformation=T)
        got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p)
        r.close()
        op = gl_parity.oracle_params(orc, sc, T, cull, subpixel_bits=4)
        want = orc.render_stereo_gl(op, d, c, near_clip=True, samples=samples, pattern=1, resolve=1)
        _compare(got, want, W, f"gl fixture cull={cull} samples={samples}")
        mask = got["mask"].cpu().numpy()
        key = f"left_c{int(cull)}s{4 if samples else 0}_mask"
        assert np.array_equal(mask[:, :W], g[key]), (key, int((mask[:, :W] != g[key]).sum()))


# ------------------------------------------------------------------------------------------------ 3. the gate changes nothing elsewhere
def test_near_clip_is_byte_identical_where_nothing_straddles(mods):
    """Benchmark frames (mesh, posed mesh, convergence), frames posed in front of the camera, and points mode with Z = 0 patches
    (where the switch changes nothing and refuses nothing): every output equals the default render's."""
    _lib, sr, synthetic = mods
    W, H, N = 320, 180, 4
    d, c = synthetic.SyntheticScene(W, H, config_id=2).clip(N)
    dz, cz = _scene(synthetic, W, H, 4)
    cases = [("mesh", dict(), [dict(xfov=45.0)] * N, d, c),
             ("posed mesh", dict(), [dict(xfov=45.0, transformation=T) for T in synthetic.synthetic_pose_track(N)], d, c),
             ("convergence", dict(infill_mask=True, dont_place_points_in_edges=True), [dict(xfov=45.0, convergence_distance=2.5)] * N, d, c),
             ("in front", dict(remove_edges=True, dont_place_points_in_edges=True), [dict(xfov=45.0, transformation=_tz(1.0))] * N, d, c),
             ("points", dict(render_as_pointcloud=True, infill_mask=True), [dict(xfov=45.0, transformation=_tz(-0.5))] * N,
              np.stack([dz] * N), np.stack([cz] * N))]
    for name, kw, fps, dd, cc in cases:
        outs = []
        for near_clip in (False, True):
            r = sr.StereoRerenderer(W, H, pupillary_distance=65, near_clip=near_clip, **kw)
            p = [r.frame_params(**fp) for fp in fps]
            extra = dict(want_depth=True, want_seed=True, want_maskbits=True) if name == "points" else {}
            got = r.render(torch.from_numpy(np.ascontiguousarray(dd)).cuda(), torch.from_numpy(np.ascontiguousarray(cc)).cuda(), p,
                           want_hole_counts=True, **extra)
            outs.append({k: v.cpu().numpy() for k, v in got.items()})
            r.close()
        for k in outs[0]:
            assert np.array_equal(outs[0][k], outs[1][k]), (name, k)


# ------------------------------------------------------------------------------------------------ 4. batches and layouts
@pytest.mark.parametrize("samples", [0, 4])
def test_near_clip_batch_mixed_frames_padded_pitches(mods, orc, samples):
    """9 frames in one call -- straddling and clean frames of every kind mixed, padded rows, separate eye buffers, a workspace budget
    of 1 MiB (several launch sets) -- each equals its oracle render; hole counts equal the masks."""
    _lib, sr, synthetic = mods
    W, H, N = 120, 66, 9
    pad_in, pad_out, pad_m = 21, 15, 5
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, near_clip=True, samples=samples, remove_edges=True,
                            dont_place_points_in_edges=True, workspace_mib=1)
    kinds = ["pure", "pose2", "clean", "convergence", "clean_pose", "pose5", "pose_patch", "clean", "pure"]
    scenes, params, Ts = [], [], []
    for f, kind in enumerate(kinds):
        if kind.startswith("clean"):
            conv, T, patch, cfg = None, synthetic.synthetic_pose_track(N)[f] if kind == "clean_pose" else None, False, 2
        else:
            conv, T, patch, cfg = _kind(synthetic, kind)
        scenes.append(_scene(synthetic, W, H, 20 + f, patch=patch, config_id=cfg))
        params.append(r.frame_params(xfov=40.0 + 3 * f, convergence_distance=conv, transformation=T))
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
    for _ in range(2):                       # (twice: the key planes must be left empty for the next call)
        r.ctx.check(_lib.load().mdvt_render_stereo_batch(r.ctx.handle, N, arr, C.byref(io), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    assert r.ctx.workspace_bytes() >= 16 * W * H, "the key planes are reported as workspace"
    cnt = counts.cpu().numpy()
    for f in range(N):
        want = _oracle(orc, r, params[f], scenes[f][0], scenes[f][1], Ts[f])
        for eye, k in ((0, "l"), (1, "r")):
            name = ("left", "right")[eye]
            rgb = outs[k][f, :, :3 * W].cpu().numpy().reshape(H, W, 3)
            m = masks[k][f, :, :W].cpu().numpy()
            assert np.array_equal(rgb, want[name + "_rgb"]) and np.array_equal(m, want[name + "_mask"]), (kinds[f], f, name)
            assert (outs[k][f, :, 3 * W:] == 7).all() and (masks[k][f, :, W:] == 7).all(), "padding must stay untouched"
            assert int(cnt[f, eye]) == int(m.sum()) // 255, (kinds[f], f, name, "hole count")
    r.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_near_clip_refusals(mods):
    _lib, sr, synthetic = mods
    W, H = 64, 48
    L = _lib.load()
    ctx = _lib.Context(torch.cuda.current_device(), W, H)
    for v in (2, -1, 7):
        assert L.mdvt_set_near_clip(ctx.handle, v) == MDVT_ERR_INVALID_ARG
        assert "near_clip" in L.mdvt_last_error(ctx.handle).decode()
    assert L.mdvt_set_near_clip(ctx.handle, 1) == 0 and L.mdvt_set_near_clip(ctx.handle, 0) == 0
    ctx.close()
    d, c = _scene(synthetic, W, H, seed=1)
    d, c = torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()
    r = sr.StereoRerenderer(W, H, near_clip=True, infill_mask=True)                 # edge points on (sr:589)
    with pytest.raises(_lib.MdvtError, match="edge points") as e:
        r.render(d, c, r.frame_params(xfov=45.0))
    assert e.value.code == MDVT_ERR_UNSUPPORTED and "near-plane clipping" in str(e.value)
    r.close()
    r = sr.StereoRerenderer(W, H, near_clip=True, infill_mask=True, dont_place_points_in_edges=True)
    p = r.frame_params(xfov=45.0)
    for kw, word in ((dict(want_depth=True), "depth planes"), (dict(want_seed=True), "seed images"),
                     (dict(want_maskbits=True), "packed mask bits"), (dict(want_maskbits=True, want_mask=False), "packed mask bits")):
        with pytest.raises(_lib.MdvtError, match=word) as e:
            r.render(d, c, p, **kw)
        assert e.value.code == MDVT_ERR_UNSUPPORTED, kw
    r.render(d, c, p, want_hole_counts=True)                                    # ... and the context still renders
    r.close()
    r = sr.StereoRerenderer(W, H, near_clip=True, render_as_pointcloud=True, infill_mask=True)   # points: nothing refused
    r.render(d, c, r.frame_params(xfov=45.0), want_depth=True, want_seed=True, want_maskbits=True)
    r.close()


# ------------------------------------------------------------------------------------------------ 6. randomised sweep
def nc_sweep_cases(synthetic):
    """MDVT_NC_SWEEP_SEED / MDVT_NC_SWEEP_CASES widen the sweep (soaks) without touching the default."""
    rng = np.random.default_rng(int(os.environ.get("MDVT_NC_SWEEP_SEED", "20261016")))
    sizes = [(2, 2), (3, 2), (5, 3), (8, 8), (17, 9), (36, 20), (61, 33), (100, 31), (128, 16)]
    for case in range(int(os.environ.get("MDVT_NC_SWEEP_CASES", "40"))):
        W, H = sizes[int(rng.integers(len(sizes)))]
        code = rng.integers(0, 65536, (H, W)).astype(np.uint32)
        style = int(rng.integers(4))
        if style == 0:                                   # smooth plane with holes of code 0
            code = (2000 + 40 * np.arange(W)[None, :] + 7 * np.arange(H)[:, None]).astype(np.uint32)
            code[rng.random((H, W)) < 0.1] = 0
        elif style == 1:                                 # very near content with code 0 here and there
            code = rng.integers(0, 4, (H, W)).astype(np.uint32)
        elif style == 2:                                 # random codes, 30 % zero
            code[rng.random((H, W)) < 0.3] = 0
        depth_rgb = np.zeros((H, W, 3), np.uint8)
        depth_rgb[..., 0], depth_rgb[..., 2] = (code >> 8) & 0xFF, code & 0xFF
        color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        samples = int(rng.choice([0, 1, 4]))
        kw = dict(pupillary_distance=int(rng.choice([0, 30, 63, 400])), max_depth=int(rng.choice([5, 20, 100, 655])),
                  cull=int(rng.integers(3)), subpixel_bits=int(rng.choice([0, 4])), samples=samples,
                  sample_pattern=int(rng.integers(2)) if samples == 4 else 0, sample_resolve=int(rng.integers(2)) if samples == 4 else 0)
        if rng.integers(2):
            kw.update(remove_edges=True, dont_place_points_in_edges=True)
        tz = float(rng.choice([0.0, -0.5, -2.0, 0.3]))
        T = None if tz == 0.0 and rng.integers(2) else _tz(tz)
        if T is not None and rng.integers(2):
            a = float(rng.uniform(-0.5, 0.5))
            T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        conv = float(rng.choice([1.0, 2.5])) if rng.integers(3) == 0 else None
        yield dict(case=case, depth_rgb=depth_rgb, color=color, T=T, conv=conv, xfov=float(rng.choice([20.0, 45.0, 90.0])), kw=kw,
                   style=style)


def test_near_clip_randomised_sweep(mods, orc):
    _lib, sr, synthetic = mods
    for cs in nc_sweep_cases(synthetic):
        d, c = cs["depth_rgb"], cs["color"]
        H, W = d.shape[:2]
        r = sr.StereoRerenderer(W, H, near_clip=True, **cs["kw"])
        p = r.frame_params(xfov=cs["xfov"], convergence_distance=cs["conv"], transformation=cs["T"])
        got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), p, want_hole_counts=True)
        tag = f"nc-sweep#{cs['case']} {W}x{H} style={cs['style']} conv={cs['conv']} T={cs['T'] is not None} {cs['kw']}"
        _compare(got, _oracle(orc, r, p, d, c, cs["T"]), W, tag)
        m, cnt = got["mask"].cpu().numpy(), got["hole_counts"].cpu().numpy()
        assert int(cnt[0]) == int(m[:, :W].sum()) // 255 and int(cnt[1]) == int(m[:, W:].sum()) // 255, tag + " counts"
        r.close()


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_cli_near_clip_end_to_end(mods, tmp_path):
    _lib, sr, synthetic = mods
    W, H, N = 96, 54, 3
    depth, color = synthetic.SyntheticScene(W, H, seed=8, n_fg=5).clip(N)
    depth[:, 10:20, 30:45] = 0                        # Z = 0 patches: straddling triangles in every frame
    dp, cp = str(tmp_path / "d.npy"), str(tmp_path / "c.npy")
    np.save(dp, depth)
    np.save(cp, color)
    rc = sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "50", "--pupillary_distance", "65", "--batch", "2", "--near_clip"])
    assert rc == 0
    sbs, mask = np.load(dp + "_stereo.npy"), np.load(dp + "_stereo.npy_holemask.npy")
    r = sr.StereoRerenderer(W, H, pupillary_distance=65, near_clip=True)
    p = r.frame_params(xfov=50.0)
    got = r.render(torch.from_numpy(np.ascontiguousarray(depth)).cuda(), torch.from_numpy(np.ascontiguousarray(color)).cuda(), [p] * N)
    assert np.array_equal(sbs, got["sbs"].cpu().numpy())
    assert np.array_equal(mask.reshape(N, H, 2 * W), got["mask"].cpu().numpy())
    r.close()
    r = sr.StereoRerenderer(W, H, pupillary_distance=65)
    off = r.render(torch.from_numpy(np.ascontiguousarray(depth)).cuda(), torch.from_numpy(np.ascontiguousarray(color)).cuda(), [p] * N)
    assert not np.array_equal(sbs, off["sbs"].cpu().numpy()), "the flag must reach the renderer"
    r.close()
    os.remove(dp + "_stereo.npy")
    with pytest.raises(ValueError, match="dont_place_points_in_edges"):
        sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "50", "--near_clip", "--infill_mask"])
    assert not os.path.exists(dp + "_stereo.npy")
