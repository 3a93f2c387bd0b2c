"""The footprint of include/mdvt_geometry.h's two entry points, with the arenas of tests/footprint.py (poison and complement, odd
bases, padded rows, gaps between frames): exactly the stated entries change -- 3 N doubles of vertices, M triples, U entries of the
three vertex lists, 2 n_frames words of counts --, entries past a count keep their poison, a refused call leaves everything as it
was (one case per refusal the header lists), and frames and buffers more than 4 GiB apart are addressed at 64 bits."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import geometry_cases as gc
import geometry_ref as gr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ENTRY, GREY = "mdvt_export_geometry_batch", "mdvt_depth_grey_batch"
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib
    return _lib


@pytest.fixture()
def own_tally():
    try:
        yield
    finally:
        fp.TALLY.pop(ENTRY, None)                      # test_gpu_footprint.py's table lists include/mdvt.h's entry points only
        fp.TALLY.pop(GREY, None)


def _vp(a):
    return C.c_void_p(a.ptr)


# what a refused case changes: name -> (status, how)
REFUSALS = {
    "null params": INVALID, "null opts": INVALID, "null io": INVALID, "null depth_rgb": INVALID, "null counts": INVALID,
    "point_rgb without color_rgb": INVALID, "points stride": INVALID, "point_rgb stride": INVALID, "used_index stride": INVALID,
    "vertices misaligned": INVALID, "points misaligned": INVALID, "triangles misaligned": INVALID, "used_index misaligned": INVALID,
    "counts misaligned": INVALID, "n_frames 0": INVALID, "depth pitch": INVALID, "color pitch": INVALID, "depth stride": INVALID,
    "decode 2": UNSUPPORTED, "reserved": UNSUPPORTED, "pose not affine": UNSUPPORTED,
}


def test_export_geometry_footprint(lib, own_tally):
    L = lib.load()
    refusals = sorted(REFUSALS)
    for k, (rng, lays) in enumerate(fp.layout_sweep(4, 1620)):
        W = max(2, int(rng.choice((2, 3, 5, 8, 17, 33, 64, 129, 257))))
        H = int(rng.choice((2, 3, 5, 13, 40, 67)))
        N = 1 + k % 3
        decode, remove = k % 2, 1 if k % 4 else 0
        # one frame's depth for the whole batch -- the same U and M in every frame, so that a list's payload is a rectangle -- under
        # different poses and colours
        frame = gc.scene(rng, H, W, k, split=not decode)
        depth = np.stack([frame] * N)
        color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        Ts = gc.poses(3)[3 - N:]
        scales = [0.8] * N
        K = gc.K_of(W, H)
        refs = [gr.export(depth[f], K, decode=decode, remove_edges=remove, T=Ts[f], depth_scale=scales[f], color_rgb=color[f]) for f in range(N)]
        U, M = refs[0].counts
        if U == 0 or M == 0:
            continue
        npx, ntri = W * H, 2 * (W - 1) * (H - 1)
        arr = gc.params_of(lib, K, scales, Ts)
        ctx = gc.make_context(lib, W, H)
        ld, lc, lrgb = lays.u8(), lays.u8(), lays.u8()
        gap = int(rng.choice((0, 0, 8, 40)))
        try:
            def body(run, bad=None):
                d = run.inp("depth", depth.reshape(N, H, 3 * W), ld)
                c = run.inp("color", color.reshape(N, H, 3 * W), lc)
                # (a list's frames are a full list + gap apart; the payload is what the call states it writes)
                outs = {}
                for name, n, cap, base in (("vertices", npx, npx, 8 * (k % 2)), ("triangles", M, ntri, 4 * (k % 4)), ("used_index", U, npx, 4 * ((k + 1) % 4)),
                                           ("points", U, npx, 8 * ((k + 1) % 2)), ("point_rgb", U, npx, lrgb.base)):
                    item = gc.ITEM[name]
                    stride = cap * item + gap * (1 if name == "point_rgb" else 8)
                    stride += -stride % (1 if name == "point_rgb" else 8)
                    a = fp.Arena(1, n * item, n * item, N, stride, base + (1 if bad == name + " misaligned" else 0), seed=run.seed * 1000 + len(run.arenas),
                                 complement=run.complement, device=run.device, name=f"{ENTRY} {name}")
                    run.arenas[name] = outs[name] = a
                cnt = run.out("counts", 1, 8 * N, 1, fp.Layout(4 * (k % 3) + (1 if bad == "counts misaligned" else 0)))
                opts = lib.MdvtGeometryOpts(decode=2 if bad == "decode 2" else decode, remove_edges=remove, max_depth=100.0)
                if bad == "reserved":
                    opts.reserved[1] = 1
                io = lib.MdvtGeometryIO()
                io.depth_rgb, io.depth_pitch, io.depth_stride = d.ptr, d.pitch, d.stride
                io.color_rgb, io.color_pitch, io.color_stride = c.ptr, c.pitch, c.stride
                for name, a in outs.items():
                    setattr(io, name, a.ptr)
                    setattr(io, {"used_index": "used_stride"}.get(name, name + "_stride"), a.stride)
                io.counts = cnt.ptr
                n_frames, p = N, arr
                if bad == "null depth_rgb":
                    io.depth_rgb = None
                elif bad == "null counts":
                    io.counts = None
                elif bad == "point_rgb without color_rgb":
                    io.color_rgb = None
                elif bad == "points stride":
                    n_frames, io.points_stride = 2, 24 * npx - 8
                elif bad == "point_rgb stride":
                    n_frames, io.point_rgb_stride = 2, 3 * npx - 1
                elif bad == "used_index stride":
                    n_frames, io.used_stride = 2, 4 * npx - 4
                elif bad == "n_frames 0":
                    n_frames = 0
                elif bad == "depth pitch":
                    io.depth_pitch = 3 * W - 1
                elif bad == "color pitch":
                    io.color_pitch = 3 * W - 1
                elif bad == "depth stride":
                    n_frames, io.depth_stride = 2, d.pitch * H - 1
                elif bad == "pose not affine":
                    p = gc.params_of(lib, K, scales, [np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1e-3, 1.0]])] * N)
                if bad in ("points stride", "point_rgb stride", "used_index stride", "depth stride") and N < 2:
                    p = gc.params_of(lib, K, [0.8, 0.8], [None, None])       # (a refusal: the second frame is never reached)
                rc = L.mdvt_export_geometry_batch(ctx.handle, n_frames, None if bad == "null params" else p,
                                                  None if bad == "null opts" else C.byref(opts), None if bad == "null io" else C.byref(io), None)
                if bad is None:
                    ctx.check(rc)
                return rc
            tag = f"{W}x{H} x{N} decode={decode} remove_edges={remove} {ld} {lc} gap {gap}"
            out = fp.twice(ENTRY, lambda run: (body(run), None)[1], seed=k, what=tag)
            fp.accepted(ENTRY)
            counts = np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(N, 2)
            assert np.array_equal(counts, [[U, M]] * N), f"{tag}: {counts}"
            for name in gc.OUTPUTS:
                for f in range(N):
                    want = np.ascontiguousarray(getattr(refs[f], name), gc.DTYPE[name])
                    assert out[name][f].tobytes() == want.tobytes(), f"{tag}: {name} of frame {f}"
            for bad in (refusals[k % len(refusals)], refusals[(k + 7) % len(refusals)], refusals[(k + 14) % len(refusals)]):
                fp.refused(ENTRY, lambda run: body(run, bad=bad), REFUSALS[bad], seed=k)
        finally:
            ctx.close()
    fp.finish_entry(ENTRY)
    t = fp.tally(ENTRY)
    assert t["accepted"] >= 10 and t["refused"] >= 21 and t["outside_bytes"] >= 2 * 4096 * t["accepted"]


def test_refused_frame_sizes(lib, own_tally):
    """A frame below 2 x 2 (invalid) and one of more than 2^28 vertices (unsupported): refused before anything is written."""
    L = lib.load()
    for (W, H), status in (((1, 5), INVALID), ((7, 1), INVALID), ((32768, 16384), UNSUPPORTED)):
        ctx = gc.make_context(lib, W, H)
        try:
            def body(run):
                d = run.inp("depth", np.zeros((1, 2, 3 * 8), np.uint8))
                v = run.out("vertices", 1, 96, 1, fp.Layout(8))
                cnt = run.out("counts", 1, 8, 1, fp.Layout(4))
                opts = lib.MdvtGeometryOpts(decode=0, remove_edges=1, max_depth=100.0)
                io = lib.MdvtGeometryIO()
                io.depth_rgb, io.depth_pitch, io.depth_stride = d.ptr, 3 * W, 3 * W * H
                io.vertices, io.vertices_stride, io.counts = v.ptr, 24 * W * H, cnt.ptr
                return L.mdvt_export_geometry_batch(ctx.handle, 1, gc.params_of(lib, gc.K_of(8, 8), [1.0], [None]), C.byref(opts), C.byref(io), None)
            fp.refused(ENTRY, body, status)
        finally:
            ctx.close()


def test_depth_grey_footprint(lib, own_tally):
    L = lib.load()
    for k, (rng, lays) in enumerate(fp.layout_sweep(2, 1621)):
        W, H, N = int(rng.choice(fp.WIDTHS)), int(rng.choice((1, 2, 5, 13))), 1 + k % 3
        bits, max_depth = (16, 8)[k % 2], (100.0, 20.0)[(k // 2) % 2]
        depth = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        depth[rng.random((N, H, W)) < 0.1, :2] = 255                 # (codes that saturate among them)
        want = np.stack([gr.grey(depth[f], max_depth, bits)[2] for f in range(N)])
        row = (2 if bits == 16 else 3) * W
        ld = lays.u8()
        lo = lays.u8()
        if bits == 16:
            lo = fp.Layout(lo.base & ~1, lo.pad + lo.pad % 2, lo.gap + lo.gap % 2)
        ctx = gc.make_context(lib, W, H)
        try:
            def body(run, bad=None):
                d = run.inp("depth", depth.reshape(N, H, 3 * W), ld)
                lay = fp.Layout(lo.base + 1, lo.pad, lo.gap) if bad == "odd" else lo
                o = run.out("grey", H, row, N, lay)
                rc = L.mdvt_depth_grey_batch(ctx.handle, 0 if bad == "n" else N, _vp(d), 3 * W - 1 if bad == "pitch" else d.pitch, d.stride, max_depth,
                                             12 if bad == "bits" else bits, _vp(o), row - 1 if bad == "out_pitch" else o.pitch, o.stride, None)
                if bad is None:
                    ctx.check(rc)
                return rc
            tag = f"{W}x{H} x{N} bits={bits} {ld} {lo}"
            out = fp.twice(GREY, lambda run: (body(run), None)[1], seed=k, what=tag)
            fp.accepted(GREY)
            assert out["grey"].tobytes() == want.tobytes(), tag
            for bad in ("n", "pitch", "bits", "out_pitch") + (("odd",) if bits == 16 else ()):
                if k % 4 == 0:
                    fp.refused(GREY, lambda run: body(run, bad=bad), INVALID, seed=k)
        finally:
            ctx.close()
    fp.finish_entry(GREY)


def test_frames_and_lists_more_than_4_gib_apart(lib):
    """Two 8 x 2 depth frames 2^32 + 48 bytes apart, their vertices 2^32 + 2^16 bytes apart, and the points buffer more than 4 GiB
    behind the vertices: every offset is taken at 64 bits."""
    W, H, N = 8, 2, 2
    rng = np.random.default_rng(5)
    depth = np.stack([gc.scene(rng, H, W, f, split=True) for f in range(N)])
    color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    K, Ts = gc.K_of(W, H), gc.poses(2)
    refs = [gr.export(depth[f], K, decode=0, remove_edges=1, T=Ts[f], color_rgb=color[f]) for f in range(N)]
    assert refs[0].counts[0] > 0
    free, _total = torch.cuda.mem_get_info()
    need = (1 << 32) + (1 << 21)
    assert free > need + (1 << 30), "less than 5 GiB free on the device"
    slab = torch.empty(need, dtype=torch.uint8, device="cuda")
    ctx = gc.make_context(lib, W, H)
    try:
        d_stride, v_at, v_stride, p_at = (1 << 32) + 48, 8192, (1 << 32) + (1 << 16), (1 << 32) + (1 << 19)
        for at in (0, d_stride, v_at, v_at + v_stride, p_at):
            slab[max(0, at - 4096):at + 8192].fill_(gc.POISON)
        for f in range(N):
            slab[f * d_stride:f * d_stride + 48].copy_(torch.from_numpy(depth[f].reshape(-1)).cuda())
        c = torch.from_numpy(color).cuda()
        counts = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        used = torch.full((N, W * H), -1, dtype=torch.int32, device="cuda")
        io = lib.MdvtGeometryIO()
        io.depth_rgb, io.depth_pitch, io.depth_stride = slab.data_ptr(), 3 * W, d_stride
        io.color_rgb, io.color_pitch, io.color_stride = c.data_ptr(), 3 * W, 3 * W * H
        io.vertices, io.vertices_stride = slab.data_ptr() + v_at, v_stride
        io.points, io.points_stride = slab.data_ptr() + p_at, 24 * W * H
        io.used_index, io.used_stride = used.data_ptr(), 4 * W * H
        io.counts = counts.data_ptr()
        assert io.points - io.vertices > (1 << 32)
        opts = lib.MdvtGeometryOpts(decode=0, remove_edges=1, max_depth=100.0)
        ctx.call(ENTRY, N, gc.params_of(lib, K, [1.0] * N, Ts), C.byref(opts), C.byref(io), lib.stream_arg(slab.device))
        torch.cuda.synchronize()
        for f in range(N):
            U, M = refs[f].counts
            assert counts[f].tolist() == [U, M]
            got_v = slab[v_at + f * v_stride:v_at + f * v_stride + 24 * W * H].cpu().numpy()
            assert got_v.tobytes() == refs[f].vertices.tobytes(), f"vertices of frame {f}"
            at = p_at + f * 24 * W * H
            assert slab[at:at + 24 * U].cpu().numpy().tobytes() == refs[f].points.tobytes(), f"points of frame {f}"
            assert np.all(slab[at + 24 * U:at + 24 * W * H].cpu().numpy() == gc.POISON)
            assert np.array_equal(used[f, :U].cpu().numpy(), refs[f].used_index) and np.all(used[f, U:].cpu().numpy() == -1)
        # and nothing around the far regions
        assert np.all(slab[v_at + 24 * W * H:v_at + 24 * W * H + 4096].cpu().numpy() == gc.POISON)
        assert np.all(slab[d_stride + 48:d_stride + 4096].cpu().numpy() == gc.POISON)
    finally:
        ctx.close()
        del slab
        torch.cuda.empty_cache()
