"""mdvt_view_centers (include/mdvt_view.h) and view_depthfile.centers against tests/view_ref.py, bit for bit, at sizes that cross the
summation's seams -- a tiny input, less than one chunk of 8192, one chunk and a tail at an odd width, two chunks and a tail of one
leaf --, with and without a pose, in mesh and points mode, with parked vertices, depth code 0, batches, padded rows, another stream
and a scratch block that has grown in between; then the entry point's footprint with the arenas of tests/footprint.py."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import view_ref as vr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENTRY = "mdvt_view_centers"
INVALID = -1
SIZES = [(8, 2), (96, 64), (250, 37), (128, 129)]
MODES = {"mesh": dict(render_as_pointcloud=False), "points": dict(render_as_pointcloud=True),
         "points_parked": dict(render_as_pointcloud=True, remove_edges=True), "mesh_edges": dict(remove_edges=True)}


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, view_depthfile
    return _lib, stereo_rerender, view_depthfile


def depth_frames(rng, N, H, W):
    """RGB-coded depth: a tilted background, a near box with a depth step at its rim (triangles for the 89-degree filter), noise in
    the low byte, a few pixels of depth code 0."""
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((N, H, W, 3), np.uint8)
    for f in range(N):
        code = (9000 + 40 * x + 25 * y + 700 * f).astype(np.int64)
        x0, y0 = (W // 4 + f) % max(W - 2, 1), (H // 3 + f) % max(H - 1, 1)
        code[y0:y0 + max(H // 3, 1), x0:x0 + max(W // 3, 1)] = 1500 + 100 * f
        code = (code + rng.integers(0, 64, (H, W))) & 0xFFFF
        code[rng.random((H, W)) < 0.02] = 0
        code[0, 0] = 0
        out[f, ..., 0] = out[f, ..., 1] = code >> 8
        out[f, ..., 2] = code & 0xFF
    return out


def poses(n):
    """None, then rigid poses that differ per frame."""
    out = [None]
    for k in range(1, n):
        a = 0.07 * k
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        T[:3, 3] = [0.05 * k, -0.02 * k, 0.11 * k]
        out.append(T)
    return out


def same_bits(got, want):
    return np.ascontiguousarray(got, np.float64).tobytes() == np.ascontiguousarray(want, np.float64).tobytes()


_REF = {}


def case(mods, size, mode):
    """Three frames of one size and mode, their parameter records and the reference centres -- computed once."""
    key = (size, mode)
    if key not in _REF:
        _lib, sr, _vd = mods
        W, H = size
        rng = np.random.default_rng(W * 1000 + H)
        depth = depth_frames(rng, 3, H, W)
        Ts = poses(3)
        params = [sr.make_frame_params(W, H, xfov=60.0, transformation=T) for T in Ts]
        K = np.array([params[0].K[k] for k in range(9)]).reshape(3, 3)
        kw = MODES[mode]
        want = np.stack([vr.center(depth[f], K, mesh=not kw.get("render_as_pointcloud", False), remove_edges=kw.get("remove_edges", False),
                                   T=Ts[f], depth_scale=params[f].depth_scale) for f in range(3)])
        _REF[key] = (depth, params, want)
    return _REF[key]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_centres_are_the_references_bits(mods, size, mode):
    _lib, sr, vd = mods
    W, H = size
    depth, params, want = case(mods, size, mode)
    assert (depth[..., 0].astype(int) << 8 | depth[..., 2] == 0).any() and params[0].depth_scale != 1.0
    if mode == "points_parked" and W > 8:
        K = np.array([params[0].K[k] for k in range(9)]).reshape(3, 3)
        P = vr.vertices(depth[0], K, mesh=False, remove_edges=True, depth_scale=params[0].depth_scale)
        assert np.all(P == vr.PARKED, axis=1).any(), "the case parks no vertex"
    r = sr.StereoRerenderer(W, H, device=0, **MODES[mode])
    try:
        d = torch.from_numpy(depth).cuda()
        got = vd.centers(d, params, r)                               # a batch of 3: no pose, two different poses
        assert got.dtype == torch.float64 and tuple(got.shape) == (3, 3)
        assert same_bits(got.cpu().numpy(), want), (got.cpu().numpy() - want)
        for f in (0, 2):                                             # frame by frame: with and without has_T
            assert same_bits(vd.centers(d[f], params[f], r).cpu().numpy(), want[f:f + 1])
        # padded rows and frames
        pad = torch.full((3, H + 1, W + 5, 3), 0xA5, dtype=torch.uint8, device="cuda")
        pad[:, :H, :W] = d
        view = pad[:, :H, :W]
        assert view.stride(1) == 3 * (W + 5) and view.stride(0) == 3 * (W + 5) * (H + 1)
        assert same_bits(vd.centers(view, params, r).cpu().numpy(), want)
        # another stream
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            on_s = vd.centers(d, params, r)
        s.synchronize()
        assert same_bits(on_s.cpu().numpy(), want)
        torch.cuda.current_stream().wait_stream(s)
    finally:
        r.close()


def test_the_same_bits_after_the_scratch_block_has_grown(mods):
    _lib, sr, vd = mods
    W, H = 250, 37
    depth, params, want = case(mods, (W, H), "points_parked")
    r = sr.StereoRerenderer(W, H, device=0, **MODES["points_parked"])
    try:
        d = torch.from_numpy(depth).cuda()
        first = vd.centers(d[1], params[1], r).cpu().numpy()
        before = r.ctx.workspace_bytes()
        big = vd.centers(torch.cat([d, d, d]), list(params) * 3, r).cpu().numpy()
        assert r.ctx.workspace_bytes() > before, "the larger call did not grow the block"
        again = vd.centers(d[1], params[1], r).cpu().numpy()
        assert same_bits(first, want[1:2]) and same_bits(again, first) and same_bits(big, np.concatenate([want] * 3))
    finally:
        r.close()


def test_a_small_budget_runs_the_batch_in_launch_sets(mods):
    """workspace_mib = 1 affords 2 frames of 800 x 500 with parking (24 B per chunk + 1 B/px each): 5 frames are three launch sets."""
    _lib, sr, vd = mods
    W, H = 800, 500
    rng = np.random.default_rng(11)
    depth = depth_frames(rng, 5, H, W)
    Ts = poses(5)
    params = [sr.make_frame_params(W, H, xfov=50.0, transformation=T) for T in Ts]
    K = np.array([params[0].K[k] for k in range(9)]).reshape(3, 3)
    want = np.stack([vr.center(depth[f], K, mesh=False, remove_edges=True, T=Ts[f], depth_scale=params[f].depth_scale) for f in range(5)])
    r = sr.StereoRerenderer(W, H, device=0, render_as_pointcloud=True, remove_edges=True, workspace_mib=1)
    try:
        got = vd.centers(torch.from_numpy(depth).cuda(), params, r).cpu().numpy()
        assert same_bits(got, want), got - want
        assert r.ctx.workspace_bytes() < 3 * W * H
    finally:
        r.close()


def test_centers_of_frames_more_than_4_gib_apart(mods):
    """Two 8 x 2 frames 2^32 + 48 bytes apart, rows 2^31 + 16 bytes apart in a second call: the offsets are taken at 64 bits."""
    _lib, sr, vd = mods
    W, H = 8, 2
    depth, params, want = case(mods, (W, H), "points_parked")
    free, _total = torch.cuda.mem_get_info()
    need = (1 << 32) + (1 << 20)
    assert free > need + (1 << 30), "less than 5 GiB free on the device"
    slab = torch.empty(need, dtype=torch.uint8, device="cuda")
    r = sr.StereoRerenderer(W, H, device=0, **MODES["points_parked"])
    try:
        d = torch.from_numpy(depth).cuda()
        out = torch.empty((2, 3), dtype=torch.float64, device="cuda")
        arr = r.pack_params(params[:2], 2)
        s = _lib.stream_arg(slab.device)
        stride = (1 << 32) + 48
        slab[:4096].fill_(0x5A)
        slab[stride - 4096:stride + 4096].fill_(0xC3)
        slab[48 * 0:48].copy_(d[0].reshape(-1))
        slab[stride:stride + 48].copy_(d[1].reshape(-1))
        r.ctx.call(ENTRY, 2, arr, slab.data_ptr(), 3 * W, stride, out.data_ptr(), s)
        assert same_bits(out.cpu().numpy(), want[:2])
        pitch = (1 << 31) + 16
        slab[pitch - 4096:pitch + 4096].fill_(0x3C)
        slab[:24].copy_(d[1, 0].reshape(-1))
        slab[pitch:pitch + 24].copy_(d[1, 1].reshape(-1))
        out.zero_()
        r.ctx.call(ENTRY, 1, r.pack_params(params[1:2], 1), slab.data_ptr(), pitch, 0, out.data_ptr(), s)
        assert same_bits(out[:1].cpu().numpy(), want[1:2])
    finally:
        r.close()
        del slab
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ footprint
def _vp(a):
    return C.c_void_p(a.ptr)


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop(ENTRY, None)                      # test_gpu_footprint.py's table lists include/mdvt.h's entry points only


def test_view_centers_footprint(mods, own_tally):
    """Exactly 3 * n_frames doubles, every one written, nothing else; no dependence on the bytes behind the first 3 W of a row; a
    refused call leaves everything as it was."""
    _lib, sr, _vd = mods
    L = _lib.load()
    for k, (rng, lays) in enumerate(fp.layout_sweep(4, 1510)):
        W = max(2, int(rng.choice(fp.WIDTHS)))
        H = int(rng.choice((2, 3, 5, 13, 40, 67)))                   # (257 x 40, 250 x 67: more than one chunk of 8192)
        N = 1 + k % 3
        mode = sorted(MODES)[k % len(MODES)]
        depth = depth_frames(rng, N, H, W)
        Ts = poses(3)[3 - N:]
        params = [sr.make_frame_params(W, H, xfov=60.0, transformation=T) for T in Ts]
        K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
        kw = MODES[mode]
        want = np.stack([vr.center(depth[f], K, mesh=not kw.get("render_as_pointcloud", False), remove_edges=kw.get("remove_edges", False),
                                   T=Ts[f], depth_scale=params[f].depth_scale) for f in range(N)])
        r = sr.StereoRerenderer(W, H, device=0, **kw)
        arr = r.pack_params(params, N)
        ld = lays.u8()
        try:
            def body(run, short=False, odd=False):
                d = run.inp("depth", depth.reshape(N, H, 3 * W), ld)
                o = run.out("centers", 1, 24 * N, 1, fp.Layout(8 * (k % 2) + (4 if odd else 0)))
                rc = L.mdvt_view_centers(r.ctx.handle, N, arr, _vp(d), 3 * W - 1 if short else d.pitch, d.stride, _vp(o), None)
                if not short and not odd:
                    r.ctx.check(rc)
                return rc
            tag = f"{W}x{H} x{N} {mode} {ld}"
            out = fp.twice(ENTRY, lambda run: (body(run), None)[1], seed=k, what=tag)
            fp.accepted(ENTRY)
            got = np.ascontiguousarray(out["centers"]).view(np.float64).reshape(N, 3)
            assert same_bits(got, want), f"{tag}: {got - want}"
            if k % 3 == 0:
                fp.refused(ENTRY, lambda run: body(run, short=True), INVALID, seed=k)
                fp.refused(ENTRY, lambda run: body(run, odd=True), INVALID, seed=k)
        finally:
            r.close()
    fp.finish_entry(ENTRY)
    t = fp.tally(ENTRY)
    assert t["accepted"] >= 10 and t["refused"] >= 4 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]
