"""mdvt_export_geometry_batch and mdvt_depth_grey_batch (include/mdvt_geometry.h) against tests/geometry_ref.py, bit for bit: every
output and counts, and the poison behind every list's end.  Sizes from 2 x 2 to a frame longer than one step of the compaction's scan,
both decodes, with and without the filter, posed and unposed frames with their own depth scales in one batch, launch sets under a
small budget, each optional output on its own, a reused workspace, two streams, and a render around an export on one context."""
import os

import numpy as np
import pytest

import geometry_cases as gc
import geometry_ref as gr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1.0, 0.75, 1.3]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib
    return _lib


def batch_of_three(W, H, decode):
    """Three frames with different content, no pose and two poses, three depth scales, a colour frame; decode 0: R != G, odd sums."""
    rng = np.random.default_rng(W * 1000 + H)
    depth = np.stack([gc.scene(rng, H, W, f, split=not decode) for f in range(3)])
    color = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    return depth, color, gc.poses(3)


@pytest.mark.parametrize("remove_edges", [0, 1], ids=["all", "filtered"])
@pytest.mark.parametrize("decode", [0, 1], ids=["cmf", "dfh"])
@pytest.mark.parametrize("size", [(2, 2), (6, 6), (33, 5), (36, 6), (257, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_output_is_the_references_bits(lib, size, decode, remove_edges):
    W, H = size
    depth, color, Ts = batch_of_three(W, H, decode)
    K = gc.K_of(W, H)
    if not decode:
        assert ((depth[..., 0].astype(int) + depth[..., 1]) % 2 == 1).all() and (depth[..., 0] != depth[..., 1]).all()
    refs = gc.reference(("three", size, decode, remove_edges), depth, K, decode=decode, remove_edges=remove_edges, Ts=Ts, depth_scales=SCALES,
                        color=color)
    if remove_edges and W > 6:
        assert len({r.counts for r in refs}) == 3, "the frames of the batch have the same counts"
        assert all(0 < r.counts[1] < 2 * (W - 1) * (H - 1) and r.counts[0] < W * H for r in refs[:1])
    ctx = gc.make_context(lib, W, H)
    try:
        out, counts = gc.export(lib, ctx, depth, K, decode=decode, remove_edges=remove_edges, Ts=Ts, depth_scales=SCALES, color=color, gap=3)
        gc.check(out, counts, refs, W, H, f"{W}x{H}")
        # frame by frame, with and without has_T, from padded rows and frames
        pad = torch.full((3, H + 1, W + 5, 3), 0x3C, dtype=torch.uint8, device="cuda")
        pad[:, :H, :W] = torch.from_numpy(depth).cuda()
        for f in (0, 2):
            out, counts = gc.export(lib, ctx, pad[f:f + 1, :H, :W], K, decode=decode, remove_edges=remove_edges, Ts=Ts[f:f + 1],
                                    depth_scales=SCALES[f:f + 1], color=color[f:f + 1])
            gc.check(out, counts, refs[f:f + 1], W, H, f"{W}x{H} frame {f} alone")
    finally:
        ctx.close()


@pytest.mark.parametrize("decode", [0, 1], ids=["cmf", "dfh"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_golden_scenes(lib, name, decode):
    g = np.load(os.path.join(REPO, "tests", "golden", "geometry.npz"))
    depth, color, K, max_depth = g[f"{name}_depth_rgb"][None], g[f"{name}_color"][None], g[f"{name}_K"], float(g[f"{name}_max_depth"][0])
    H, W = depth.shape[1:3]
    assert (W, H) == {"a": (48, 32), "b": (64, 48), "c": (40, 24)}[name]
    refs = gc.reference(("gold", name, decode), depth, K, decode=decode, remove_edges=1, max_depth=max_depth, color=color)
    if decode:                                                       # the reference's own vertices (tests/test_geometry_cpu.py holds the lists to it too)
        assert refs[0].vertices.tobytes() == g[f"{name}_pts_obo1"].tobytes()
    ctx = gc.make_context(lib, W, H)
    try:
        out, counts = gc.export(lib, ctx, depth, K, decode=decode, remove_edges=1, max_depth=max_depth, color=color)
        gc.check(out, counts, refs, W, H, f"scene {name}")
    finally:
        ctx.close()


def test_a_frame_longer_than_one_step_of_the_scan(lib):
    """1030 x 67: 69 010 vertices and 135 828 triangles.  A workgroup of the compaction takes kGeomBlock = 256 items, so a row of the
    frame spans five of them; one step of the scan takes kGeomScan = 256 workgroup totals = 65 536 items, so the vertex list needs two
    steps and the triangle list three.  The stripes remove triangles, and leave vertices unused, within eight items on both sides of
    every workgroup boundary of both lists."""
    W, H = 1030, 67
    assert W > gc.GEOM_BLOCK and W * H > gc.GEOM_BLOCK * gc.GEOM_SCAN and 2 * (W - 1) * (H - 1) > 2 * gc.GEOM_BLOCK * gc.GEOM_SCAN
    rng = np.random.default_rng(7)
    depth = gc.stripes(rng, H, W)[None]
    color = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    K, Ts = gc.K_of(W, H), gc.poses(2)[1:]
    refs = gc.reference("stripes", depth, K, decode=0, remove_edges=1, Ts=Ts, color=color)
    removed = refs[0].tri_invalid != 0
    unused = np.ones(W * H, bool)
    unused[refs[0].used_index] = False
    for flags in (removed, unused):
        assert 0.2 < flags.mean() < 0.8
        for b in range(gc.GEOM_BLOCK, flags.size - 8, gc.GEOM_BLOCK):
            assert flags[b - 8:b].any() and flags[b:b + 8].any() and not flags[b - 8:b + 8].all(), b
    ctx = gc.make_context(lib, W, H)
    try:
        out, counts = gc.export(lib, ctx, depth, K, decode=0, remove_edges=1, Ts=Ts, color=color)
        gc.check(out, counts, refs, W, H, "stripes")
    finally:
        ctx.close()


def test_nothing_kept_and_nothing_removed(lib):
    W, H = 36, 6
    K = gc.K_of(W, H)
    zero = np.zeros((1, H, W, 3), np.uint8)
    flat = gc.code_frame(np.full((H, W), 20000))[None]
    color = np.random.default_rng(3).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    ctx = gc.make_context(lib, W, H)
    try:
        refs = gc.reference("zero", zero, K, decode=0, remove_edges=1, color=color)
        assert refs[0].counts == (0, 0) and not refs[0].vertices.any()
        out, counts = gc.export(lib, ctx, zero, K, decode=0, remove_edges=1, color=color)
        gc.check(out, counts, refs, W, H, "all-zero depth")
        for name in ("triangles", "used_index", "points", "point_rgb"):
            assert np.all(out[name] == gc.POISON), f"{name} was written although U = M = 0"
        refs = gc.reference("flat", flat, K, decode=0, remove_edges=1, color=color)
        assert refs[0].counts == (W * H, 2 * (W - 1) * (H - 1))
        out, counts = gc.export(lib, ctx, flat, K, decode=0, remove_edges=1, color=color)
        gc.check(out, counts, refs, W, H, "a plane")
    finally:
        ctx.close()


def test_each_optional_output_on_its_own(lib):
    W, H = 36, 6
    depth, color, Ts = batch_of_three(W, H, 0)
    K = gc.K_of(W, H)
    refs = gc.reference(("three", (W, H), 0, 1), depth, K, decode=0, remove_edges=1, Ts=Ts, depth_scales=SCALES, color=color)
    ctx = gc.make_context(lib, W, H)
    try:
        for want in [()] + [(n,) for n in gc.OUTPUTS] + [("triangles", "points")]:
            out, counts = gc.export(lib, ctx, depth, K, decode=0, remove_edges=1, Ts=Ts, depth_scales=SCALES,
                                    color=color if "point_rgb" in want else None, want=want)
            assert sorted(out) == sorted(want)
            gc.check(out, counts, refs, W, H, f"only {want}")
    finally:
        ctx.close()


def test_a_small_budget_runs_the_batch_in_launch_sets(lib):
    """workspace_mib = 1 affords one frame of 640 x 420 (2 B per cell = 535 KB of flags and 12 KB of totals): 3 frames are three launch sets."""
    W, H = 640, 420
    rng = np.random.default_rng(11)
    depth = np.stack([gc.scene(rng, H, W, f) for f in range(3)])
    K, Ts = gc.K_of(W, H, 50.0), gc.poses(3)
    refs = gc.reference("sets", depth, K, decode=1, remove_edges=1, Ts=Ts)
    ctx = gc.make_context(lib, W, H, workspace_mib=1)
    try:
        out, counts = gc.export(lib, ctx, depth, K, decode=1, remove_edges=1, Ts=Ts, want=("triangles", "used_index", "points"))
        gc.check(out, counts, refs, W, H, "launch sets")
        assert ctx.workspace_bytes() < 2 * 2 * (W - 1) * (H - 1)
    finally:
        ctx.close()


def test_the_same_bits_from_a_reused_workspace_and_on_two_streams(lib):
    W, H = 257, 67                                                   # (34 KB of flags a frame: nine frames outgrow one frame's block)
    depth, color, Ts = batch_of_three(W, H, 1)
    K = gc.K_of(W, H)
    refs = gc.reference(("three", (W, H), 1, 1), depth, K, decode=1, remove_edges=1, Ts=Ts, depth_scales=SCALES, color=color)
    plain = gc.reference(("three", (W, H), 1, 0), depth, K, decode=1, remove_edges=0, Ts=Ts, depth_scales=SCALES, color=color)
    kw = dict(decode=1, Ts=Ts, depth_scales=SCALES, color=color)
    one = dict(decode=1, Ts=Ts[1:2], depth_scales=SCALES[1:2], color=color[1:2])
    ctx = gc.make_context(lib, W, H)
    try:
        out, counts = gc.export(lib, ctx, depth[1:2], K, remove_edges=1, **one)
        gc.check(out, counts, refs[1:2], W, H, "first")
        before = ctx.workspace_bytes()
        out, counts = gc.export(lib, ctx, np.concatenate([depth] * 3), K, remove_edges=1, decode=1, Ts=Ts * 3, depth_scales=SCALES * 3,
                                color=np.concatenate([color] * 3))
        gc.check(out, counts, refs * 3, W, H, "nine frames")
        assert ctx.workspace_bytes() > before, "the larger call did not grow the block"
        out, counts = gc.export(lib, ctx, depth, K, remove_edges=0, **kw)                  # other list lengths, no flags
        gc.check(out, counts, plain, W, H, "without the filter")
        out, counts = gc.export(lib, ctx, depth[1:2], K, remove_edges=1, **one)
        gc.check(out, counts, refs[1:2], W, H, "again")
        for k in range(2):                                           # two streams, one after the other
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            out, counts = gc.export(lib, ctx, depth, K, remove_edges=1, stream=s, **kw)
            gc.check(out, counts, refs, W, H, f"stream {k}")
            torch.cuda.current_stream().wait_stream(s)
    finally:
        ctx.close()


@pytest.mark.parametrize("max_depth", [100, 20])
@pytest.mark.parametrize("bits", [16, 8])
def test_grey_depth_of_every_code(lib, bits, max_depth):
    """Rows 0 .. 255: high byte = row, low byte = column, R = G; then four rows with R != G.  NumPy's value where it is in range,
    the type's maximum elsewhere (tests/test_geometry_cpu.py: only codes above 255^4 are)."""
    H, W = 260, 256
    rng = np.random.default_rng(bits + max_depth)
    hi, lo = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:256] = np.stack([hi, hi, lo], axis=-1)
    rgb[256:] = rng.integers(0, 256, (4, W, 3), dtype=np.uint8)
    rgb[256:, :, 1] = rgb[256:, :, 0] ^ rng.integers(1, 256, (4, W), dtype=np.uint8)
    v, ok, want = gr.grey(rgb, max_depth, bits)
    assert 0 < (~ok).sum() < ok.size // 16
    numpy_own = np.rint(gr.depth_of(rgb, 0, max_depth) * ((255 ** 2 if bits == 16 else 255) / max_depth))
    assert np.array_equal(want.reshape(H, W, -1)[..., 0][ok], numpy_own[ok].astype(want.dtype))
    frames = np.stack([rgb, rgb[::-1]])
    d = torch.full((2, H + 2, W + 3, 3), 0x77, dtype=torch.uint8, device="cuda")
    d[:, :H, :W] = torch.from_numpy(frames).cuda()
    row = (2 if bits == 16 else 3) * W
    out = torch.full((2, H, row + 8), gc.POISON, dtype=torch.uint8, device="cuda")
    ctx = gc.make_context(lib, W, H)
    try:
        ctx.call("mdvt_depth_grey_batch", 2, d.data_ptr(), d.stride(1), d.stride(0), float(max_depth), bits, out.data_ptr(), row + 8, (row + 8) * H,
                 lib.stream_arg(d.device))
        got = out.cpu().numpy()
    finally:
        ctx.close()
    assert np.all(got[:, :, row:] == gc.POISON)
    for f, w in enumerate((want, want[::-1])):
        g = np.ascontiguousarray(got[f, :, :row]).view(want.dtype).reshape(w.shape)
        assert np.array_equal(g, w), (f, np.argwhere(g != w)[:4])


def test_renders_around_an_export_on_one_context(lib):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr, view_depthfile as vd
    from oracle import c_oracle as co
    W, H, N = 96, 64, 2
    rng = np.random.default_rng(13)
    depth = np.stack([gc.scene(rng, H, W, f) for f in range(N)])
    color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    Ts = [np.eye(4)] + gc.poses(2)[1:]
    r = vd.view_renderer(W, H, device=0, remove_edges=True)
    try:
        params = [sr.make_frame_params(W, H, xfov=45.0, master_xfov=45.0, pupillary_distance=0, transformation=T) for T in Ts]
        K = np.array([params[0].K[i] for i in range(9)]).reshape(3, 3)
        d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()

        def render_ok():
            got = r.render(d, c, params, want_depth=True)
            sbs, mask, z = got["sbs"].cpu().numpy(), got["mask"].cpu().numpy(), got["depth"].cpu().numpy()
            for k in range(N):
                op = co.make_params(W, H, K, ipd_m=0.0, mode=co.MODE_MESH, remove_edges=True, edge_points=False, T=Ts[k], key_rgb=(255, 255, 255))
                want = co.render_stereo(op, depth[k], color[k], want_depth=True)
                for eye, sl in (("left", slice(0, W)), ("right", slice(W, 2 * W))):
                    assert np.array_equal(sbs[k][:, sl], want[eye + "_rgb"]) and np.array_equal(mask[k][:, sl], want[eye + "_mask"])
                    assert np.array_equal(z[k][:, sl], want[eye + "_depth"])

        refs = gc.reference("around", depth, K, decode=1, remove_edges=1, Ts=Ts, color=color)
        render_ok()
        out, counts = gc.export(lib, r.ctx, depth, K, decode=1, remove_edges=1, Ts=Ts, color=color)
        gc.check(out, counts, refs, W, H, "between renders")
        render_ok()
    finally:
        r.close()
