"""mdvt_render_view_batch (include/mdvt_view.h) and view_depthfile.render_view against the oracle: rgb with the holes set back to
black, mask and depth equal the LEFT eye of orc_render_stereo for make_params(ipd_m = 0, T = V @ T_frame, key = white), bit for bit;
in the holes rgb is the key.  Modes x remove_edges x cull at two sizes, a camera off to the side of a depth step (triangles in the
queue and in the huge list, read from the tuning library's counters), a batch longer than a launch set, stereo renders around a view
render on one context, the refusals."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

UNSUPPORTED, INVALID = -3, -1
WHITE = (255, 255, 255)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, view_depthfile
    from oracle import c_oracle
    return _lib, stereo_rerender, view_depthfile, c_oracle


def scene(rng, N, H, W, step=False):
    """Depth codes and colours: a tilted background 4 to 6 m away with a box 1.5 m away (its rim: a depth step), noise, a few pixels of
    depth code 0; no colour equals the key by accident except where the test says so."""
    y, x = np.mgrid[0:H, 0:W]
    depth = np.empty((N, H, W, 3), np.uint8)
    for f in range(N):
        code = (2700 + 6 * x + 9 * y + 40 * f).astype(np.int64)
        code[H // 4:H // 4 + H // 2, W // 3 + f:W // 3 + f + W // 4] = 1000 + 10 * f
        code = (code + rng.integers(0, 8, (H, W))) & 0xFFFF
        code[rng.random((H, W)) < 0.01] = 0
        if step:
            code[:, :W // 8] = 330                                  # a flat wall half a metre from the original viewpoint
        depth[f, ..., 0] = depth[f, ..., 1] = code >> 8
        depth[f, ..., 2] = code & 0xFF
    color = rng.integers(0, 255, (N, H, W, 3), dtype=np.uint8)      # (never 255: never the white key)
    color[:, 1, 1] = 255                                            # ... but for one drawn-white pixel: the colour-key rule marks it a hole
    return depth, color


def poses(n):
    out = []
    for k in range(n):
        a = 0.02 * k
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        T[:3, 3] = [0.01 * k, -0.02 * k, 0.03 * k]
        out.append(T)
    return out


def views_for(vd, n, cam=(0.6, 0.5, -1.2), target=(0.0, 0.1, 4.0)):
    return np.stack([vd.look_at_view(vd.camera_position(cam[0] + 0.05 * k, cam[1], cam[2]), target) for k in range(n)])


def check(mods, r, depth, color, params, Ts, views, got, *, mesh, remove_edges, cull, tag, holes=(0.02, 0.98)):
    _lib, sr, vd, co = mods
    N, H, W = depth.shape[:3]
    K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
    rgb, mask, z = got["rgb"].cpu().numpy(), got["mask"].cpu().numpy(), got["depth"].cpu().numpy()
    counts = got["hole_counts"].cpu().numpy()
    for k in range(N):
        op = co.make_params(W, H, K, ipd_m=0.0, max_depth=100.0, depth_scale=params[k].depth_scale, mode=co.MODE_MESH if mesh else co.MODE_POINTS,
                            remove_edges=remove_edges, edge_points=False, T=views[k] @ Ts[k], key_rgb=WHITE, cull=cull)
        want = co.render_stereo(op, depth[k], color[k], want_depth=True)
        hole = want["left_mask"] != 0
        assert np.array_equal(mask[k], want["left_mask"]), f"{tag} frame {k}: mask"
        assert np.array_equal(z[k], want["left_depth"]), f"{tag} frame {k}: depth"
        assert np.all(rgb[k][hole] == np.array(WHITE, np.uint8)), f"{tag} frame {k}: a hole is not the key colour"
        back = rgb[k].copy()
        back[hole] = 0
        assert np.array_equal(back, want["left_rgb"]), f"{tag} frame {k}: rgb"
        assert int(counts[k]) == int(hole.sum()), f"{tag} frame {k}: hole count"
        assert holes[0] <= hole.mean() < holes[1], f"{tag} frame {k}: {hole.mean():.3f} of the image are holes"


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("remove_edges", [False, True], ids=["", "remove_edges"])
@pytest.mark.parametrize("mesh", [True, False], ids=["mesh", "points"])
@pytest.mark.parametrize("size", [(96, 64), (250, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_view_is_the_oracles_left_eye(mods, size, mesh, remove_edges, cull):
    _lib, sr, vd, co = mods
    W, H = size
    N = 2
    rng = np.random.default_rng(W + 7 * H)
    depth, color = scene(rng, N, H, W)
    Ts = poses(N)
    views = views_for(vd, N)
    r = vd.view_renderer(W, H, device=0, render_as_pointcloud=not mesh, remove_edges=remove_edges, cull=cull)
    try:
        params = [sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=T) for T in Ts]
        assert params[0].depth_scale == 1.0
        d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        got = vd.render_view(d, c, views, params, r, want_depth=True, want_hole_counts=True)
        check(mods, r, depth, color, params, Ts, views, got, mesh=mesh, remove_edges=remove_edges, cull=cull, tag=f"{W}x{H}")
        # without the optional outputs: the same image
        only = vd.render_view(d, c, views, params, r, want_mask=False)
        assert sorted(only) == ["rgb"] and torch.equal(only["rgb"], got["rgb"])
    finally:
        r.close()


@pytest.mark.parametrize("mesh", [True, False], ids=["mesh", "points"])
def test_a_camera_off_to_the_side_of_a_depth_step(mods, mesh, monkeypatch):
    """256 x 96, the camera outside the original viewpoint and next to a depth step: right in front of a near wall beside the far
    background, so that the mesh has triangles in the queue and in the huge-triangle list -- read from the counters of the tuning
    library's queue block, not assumed."""
    _lib, sr, vd, co = mods
    monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")
    W, H = 256, 96
    rng = np.random.default_rng(5)
    depth, color = scene(rng, 1, H, W, step=True)
    Ts = [np.eye(4)]
    # the wall is flat at z = 0.5115 m: from 8 mm in front of it a cell covers a tenth of the image
    views = np.stack([vd.look_at_view(vd.camera_position(-0.185, 0.001, 0.503), (0.015, 0.05, 4.0))])
    r = vd.view_renderer(W, H, device=0, render_as_pointcloud=not mesh)
    try:
        params = [sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=Ts[0])]
        d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        got = vd.render_view(d, c, views, params, r, want_depth=True, want_hole_counts=True)
        check(mods, r, depth, color, params, Ts, views, got, mesh=mesh, remove_edges=False, cull=0, tag="side camera", holes=(0.0, 0.98))
        if mesh:
            blk, info = r.ctx.debug_read_queue_block()
            queued = int(blk[info[1]:info[1] + H].sum())
            huge = int(blk[info[3] + 2 * (1 << 17)])                 # (kHugeCap row-block entries, then the counter: mdvt_workspace.h)
            print(f"side camera: {queued} queued triangles, {huge} huge row blocks")
            assert queued > 0 and huge > 0
    finally:
        r.close()


@pytest.mark.parametrize("mesh", [True, False], ids=["mesh", "points"])
def test_a_batch_longer_than_a_launch_set(mods, mesh):
    """Five frames with their own views and workspace_mib = 1: 96 x 64 x ~90 B a slot affords one slot (mesh), the points path takes four
    frames a set -- either way more than one launch set."""
    _lib, sr, vd, co = mods
    W, H, N = 96, 64, 5
    rng = np.random.default_rng(9)
    depth, color = scene(rng, N, H, W)
    Ts = poses(N)
    views = views_for(vd, N)
    r = vd.view_renderer(W, H, device=0, render_as_pointcloud=not mesh, remove_edges=True, workspace_mib=1)
    try:
        params = [sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=T) for T in Ts]
        d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        for _ in range(2):                                           # the second call finds the key planes as the first left them
            got = vd.render_view(d, c, views, params, r, want_depth=True, want_hole_counts=True)
            check(mods, r, depth, color, params, Ts, views, got, mesh=mesh, remove_edges=True, cull=0, tag="batch of 5")
    finally:
        r.close()


@pytest.mark.parametrize("mesh", [True, False], ids=["mesh", "points"])
def test_stereo_renders_around_a_view_render_on_one_context(mods, mesh):
    _lib, sr, vd, co = mods
    W, H, N = 96, 64, 2
    rng = np.random.default_rng(13)
    depth, color = scene(rng, N, H, W)
    Ts = poses(N)
    views = views_for(vd, N)
    K = None
    r = vd.view_renderer(W, H, device=0, render_as_pointcloud=not mesh)
    try:
        params = [sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=T) for T in Ts]
        K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
        d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()

        def stereo_ok():
            got = r.render(d, c, params, want_depth=True)
            sbs, mask, z = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy(), got["depth"].cpu().numpy()
            for k in range(N):
                op = co.make_params(W, H, K, ipd_m=0.0, mode=co.MODE_MESH if mesh else co.MODE_POINTS, T=Ts[k], key_rgb=WHITE)
                want = co.render_stereo(op, depth[k], color[k], want_depth=True)
                for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                    assert np.array_equal(sbs[k][:, sl], want[eye + "_rgb"]) and np.array_equal(mask[k][:, sl], want[eye + "_mask"])
                    assert np.array_equal(z[k][:, sl], want[eye + "_depth"])

        def view_ok():
            got = vd.render_view(d, c, views, params, r, want_depth=True, want_hole_counts=True)
            check(mods, r, depth, color, params, Ts, views, got, mesh=mesh, remove_edges=False, cull=0, tag="between stereo renders")

        view_ok()                                                    # first: the context holds one eye's planes only
        one_eye = r.ctx.workspace_bytes()
        stereo_ok()
        assert r.ctx.workspace_bytes() > one_eye, "the stereo render found a second eye's planes in a context that had drawn views only"
        view_ok()
        view_ok()
        stereo_ok()
    finally:
        r.close()


def test_refused_requests_leave_everything_untouched(mods):
    _lib, sr, vd, co = mods
    W, H = 16, 8
    rng = np.random.default_rng(2)
    depth, color = scene(rng, 1, H, W)
    d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
    views = views_for(vd, 1)
    p = sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0)

    def call(r, params, **over):
        rgb = torch.full((1, H, W, 3), 0x5A, dtype=torch.uint8, device="cuda")
        mask = torch.full((1, H, W), 0x5A, dtype=torch.uint8, device="cuda")
        io = _lib.MdvtViewIO()
        io.depth_rgb, io.depth_pitch, io.depth_stride = d.data_ptr(), 3 * W, 3 * W * H
        io.color_rgb, io.color_pitch, io.color_stride = c.data_ptr(), 3 * W, 3 * W * H
        io.rgb, io.rgb_pitch, io.rgb_stride = rgb.data_ptr(), 3 * W, 3 * W * H
        io.mask, io.mask_pitch, io.mask_stride = mask.data_ptr(), W, W * H
        for k, v in over.items():
            setattr(io, k, v)
        rc = r.ctx._L.mdvt_render_view_batch(r.ctx.handle, 1, params, C.byref(io), None)
        torch.cuda.synchronize()
        assert bool((rgb == 0x5A).all()) and bool((mask == 0x5A).all()), "a refused call wrote"
        return rc

    ok = vd.view_params(p, views)
    plain = (_lib.MdvtFrameParams * 1)(p)
    cases = [(dict(remove_edges=True, dont_place_points_in_edges=False), ok, {}, UNSUPPORTED),      # edge points
             (dict(samples=4), ok, {}, UNSUPPORTED), (dict(near_clip=True), ok, {}, UNSUPPORTED),
             (dict(), plain, {}, INVALID),                                                                # has_T = 0
             (dict(), ok, dict(rgb_pitch=3 * W - 1), INVALID), (dict(), ok, dict(rgb=None), INVALID)]
    for kw, params, over, status in cases:
        r = sr.StereoRerenderer(W, H, device=0, pupillary_distance=0, **kw)
        try:
            assert call(r, params, **over) == status, (kw, over)
        finally:
            r.close()


def test_a_view_of_frames_more_than_4_gib_apart(mods):
    """Two 8 x 2 frames whose inputs AND outputs lie 2^32 + 64 bytes apart: every frame offset is taken at 64 bits."""
    _lib, sr, vd, co = mods
    W, H, N = 8, 2, 2
    rng = np.random.default_rng(21)
    depth, color = scene(rng, N, H, W)
    depth[..., 0] = depth[..., 1] = 12                               # (a tiny frame: everything about 4.7 m away, in sight)
    Ts = poses(N)
    views = np.stack([vd.look_at_view(vd.camera_position(0.02 * k, 0.01, -0.2), (0.0, 0.0, 4.7)) for k in range(N)])
    stride = (1 << 32) + 64
    need = stride + (1 << 16)
    free, _total = torch.cuda.mem_get_info()
    assert free > 4 * need + (1 << 30), "less than 18 GiB free on the device"
    slabs = {k: torch.empty(need, dtype=torch.uint8, device="cuda") for k in ("depth", "color", "rgb", "mask")}
    r = vd.view_renderer(W, H, device=0)
    try:
        params = vd.view_params([sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=T) for T in Ts], views)
        for f in range(N):
            slabs["depth"][f * stride:f * stride + 3 * W * H].copy_(torch.from_numpy(depth[f]).reshape(-1))
            slabs["color"][f * stride:f * stride + 3 * W * H].copy_(torch.from_numpy(color[f]).reshape(-1))
            for k in ("rgb", "mask"):
                slabs[k][max(0, f * stride - 4096):f * stride + 4096].fill_(0x5A)
        io = _lib.MdvtViewIO()
        io.depth_rgb, io.depth_pitch, io.depth_stride = slabs["depth"].data_ptr(), 3 * W, stride
        io.color_rgb, io.color_pitch, io.color_stride = slabs["color"].data_ptr(), 3 * W, stride
        io.rgb, io.rgb_pitch, io.rgb_stride = slabs["rgb"].data_ptr(), 3 * W, stride
        io.mask, io.mask_pitch, io.mask_stride = slabs["mask"].data_ptr(), W, stride
        r.ctx.call("mdvt_render_view_batch", N, params, C.byref(io), None)
        torch.cuda.synchronize()
        K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
        seen = 0
        for f in range(N):
            op = co.make_params(W, H, K, ipd_m=0.0, mode=co.MODE_MESH, T=views[f] @ Ts[f], key_rgb=WHITE)
            want = co.render_stereo(op, depth[f], color[f])
            rgb = slabs["rgb"][f * stride:f * stride + 3 * W * H].cpu().numpy().reshape(H, W, 3)
            mask = slabs["mask"][f * stride:f * stride + W * H].cpu().numpy().reshape(H, W)
            hole = want["left_mask"] != 0
            assert np.array_equal(mask, want["left_mask"]) and np.all(rgb[hole] == 255)
            rgb[hole] = 0
            assert np.array_equal(rgb, want["left_rgb"])
            seen += int((~hole).sum())
            assert bool((slabs["rgb"][f * stride + 3 * W * H:f * stride + 4096] == 0x5A).all()) and bool((slabs["mask"][f * stride + W * H:f * stride + 4096] == 0x5A).all())
            if f:
                assert bool((slabs["rgb"][f * stride - 4096:f * stride] == 0x5A).all()) and bool((slabs["mask"][f * stride - 4096:f * stride] == 0x5A).all())
        assert seen > 0, "nothing of the frames is in sight"
    finally:
        r.close()
        slabs.clear()
        torch.cuda.empty_cache()


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop("mdvt_render_view_batch", None)      # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def test_view_render_footprint(mods, own_tally):
    """With the poisoned arenas of tests/footprint.py: exactly the first 3 W bytes of each rgb row, W of each mask row and n_frames
    words of hole counts are written, every one of them, and nothing else; the result depends on no byte beyond the first 3 W of
    the input rows; a refused call leaves everything as it was."""
    _lib, sr, vd, co = mods
    L = _lib.load()
    entry = "mdvt_render_view_batch"
    for k, (rng, lays) in enumerate(fp.layout_sweep(2, 1520)):
        W = max(2, int(rng.choice(fp.WIDTHS)))
        H = int(rng.choice((2, 3, 5, 13)))
        if lays.vec:
            W = max(8, W & ~3)
        N = 1 + k % 2
        mesh, rm = bool(k % 2), bool((k // 2) % 2)
        depth, color = scene(rng, N, H, W)
        Ts = poses(N)
        views = views_for(vd, N)
        r = vd.view_renderer(W, H, device=0, render_as_pointcloud=not mesh, remove_edges=rm)
        params = vd.view_params([sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=T) for T in Ts], views)
        K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
        ld, lc, lr, lm = lays.u8(), lays.u8(), lays.u8(), lays.u8()
        try:
            def body(run, short=False):
                d = run.inp("depth", depth.reshape(N, H, 3 * W), ld)
                c = run.inp("color", color.reshape(N, H, 3 * W), lc)
                o = run.out("rgb", H, 3 * W, N, lr)
                m = run.out("mask", H, W, N, lm)
                h = run.out("holes", 1, 4 * N, 1, fp.Layout(4 * (k % 4)))
                io = _lib.MdvtViewIO()
                io.depth_rgb, io.depth_pitch, io.depth_stride = d.ptr, d.pitch, d.stride
                io.color_rgb, io.color_pitch, io.color_stride = c.ptr, c.pitch, c.stride
                io.rgb, io.rgb_pitch, io.rgb_stride = o.ptr, (3 * W - 1 if short else o.pitch), o.stride
                io.mask, io.mask_pitch, io.mask_stride = m.ptr, m.pitch, m.stride
                io.hole_counts = h.ptr
                rc = L.mdvt_render_view_batch(r.ctx.handle, N, params, C.byref(io), None)
                if not short:
                    r.ctx.check(rc)
                return rc
            tag = f"{W}x{H} x{N} {'mesh' if mesh else 'points'} remove_edges={rm} {ld} {lr} {lm}"
            out = fp.twice(entry, lambda run: (body(run), None)[1], seed=k, what=tag)
            fp.accepted(entry)
            rgb = np.ascontiguousarray(out["rgb"]).reshape(N, H, W, 3)
            mask = np.ascontiguousarray(out["mask"]).reshape(N, H, W)
            holes = np.ascontiguousarray(out["holes"]).view(np.uint32).reshape(N)
            for f in range(N):
                op = co.make_params(W, H, K, ipd_m=0.0, mode=co.MODE_MESH if mesh else co.MODE_POINTS, remove_edges=rm, edge_points=False,
                                    T=views[f] @ Ts[f], key_rgb=WHITE)
                want = co.render_stereo(op, depth[f], color[f])
                hole = want["left_mask"] != 0
                back = rgb[f].copy()
                back[hole] = 0
                assert np.array_equal(mask[f], want["left_mask"]) and np.array_equal(back, want["left_rgb"]), tag
                assert np.all(rgb[f][hole] == 255) and int(holes[f]) == int(hole.sum()), tag
            if k % 4 == 0:
                fp.refused(entry, lambda run: body(run, short=True), INVALID, seed=k)
        finally:
            r.close()
    fp.finish_entry(entry)
    t = fp.tally(entry)
    assert t["accepted"] >= 10 and t["refused"] >= 3 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
