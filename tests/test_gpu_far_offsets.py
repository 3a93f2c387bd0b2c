"""Every entry point with frames and rows more than 4 GiB apart (tests/footprint.py, "far layouts"): through the raw C ABI, every
buffer a lane of one slab, tiny frames 2^31 + delta bytes apart (far stride), rows 2^29 + delta bytes apart (far pitch), or the
buffers of one call more than 4 GiB apart (far base).  The header takes pitches, strides and offsets as size_t / uint64_t: a far
layout either gives the reference's bytes -- the same reference tests/test_gpu_footprint.py uses, every comparison is equality -- or
is refused untouched with the documented status.  Every address a 32-bit slip could compute is a watched window of the slab
(tests/test_far_arena_cpu.py shows on modelled kernels that each slip is flagged), so a defect is a changed byte or a wrong payload.
Each case runs on the poison and on its complement; every frame of a batch has its own content.

The case bodies, references and comparisons are those of tests/test_gpu_footprint.py: the render's RenderCase, and the stand-alone
entry points' own tests, run here with far arenas (fp.far), on a sweep of two or six layouts and on the sizes of this file."""
import ctypes as C

import numpy as np
import pytest

import convergence_ref as cr
import footprint as fp
import test_gpu_footprint as tgf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INVALID, UNSUPPORTED = -1, -3
ODD, VEC = (1, 3, 1), (4, 4, 4)                   # (base, pad, gap) of the byte-path layout and of the vector-eligible one
FAMILIES = sorted(tgf.FAMILIES)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, synthetic
    return _lib, stereo_rerender, synthetic


@pytest.fixture(scope="module")
def slab(mods):
    """One slab for the module.  The one permitted skip: less than twice the slab free on the device."""
    free, total = torch.cuda.mem_get_info()
    print(f"\nslab {fp.SLAB_BYTES} bytes, {free} of {total} bytes free on the device")
    reason = fp.Slab.skip_reason()
    if reason:
        pytest.skip(reason)
    s = fp.Slab()
    yield s
    del s.buf
    torch.cuda.empty_cache()


def _lays(rng, vec):
    return fp.Layouts(rng, VEC if vec else ODD, vec=vec)


def _size(vec, k, heights=(9, 11)):
    """W in {36, 64} on a vector-eligible layout, {33, 37} on the byte path; H in {9, 11}: no multiple of the band heights."""
    return ((36, 64) if vec else (33, 37))[k % 2], heights[(k // 2) % len(heights)]


def _vp(a):
    return C.c_void_p(a if isinstance(a, int) else a.ptr)


# ------------------------------------------------------------------------------------------------------------------ render
def _render(mods, orc, monkeypatch, slab, family, far, vec, W, H, N, sbs, seed, want=None, single=False, **kw):
    """One RenderCase on a far layout: all outputs the family supports (or `want`), compared with the oracle frame by frame."""
    if family == "mesh_conv":
        monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")
        monkeypatch.setenv("MDVT_MESH_CONV", "1")
    rng = np.random.default_rng(seed)
    cs = tgf.RenderCase(mods, family, rng, _lays(rng, vec), W, H, N, sbs=sbs, force_batch=not single, **kw)
    assert cs.entry == ("mdvt_render_stereo" if single else "mdvt_render_stereo_batch")
    full = ("mask",) + cs.optional if want is None else want
    tag = f"{cs.tag()} [far {far.kind}, apart {far.apart}]"
    try:
        with fp.far(far):
            out = fp.twice(cs.entry, cs.body(full), seed=seed, what=tag)
            lanes = list(fp.LAST_RUN)
        cs.compare(out, [cs.reference(orc, f) for f in range(N)], full, tag)
        assert cs.vec4 == bool(vec), f"{tag}: plan.vec4 is {cs.vec4} on a layout made for the {'vector' if vec else 'byte'} path"
        big = [a for a in lanes if (far.kind == "stride" and a.stride > 1 << 30) or (far.kind == "pitch" and a.pitch > 1 << 29)]
        assert len(big) >= 3, tag
        return cs, lanes
    finally:
        cs.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_render_batch_far_stride(mods, orc, monkeypatch, slab, family):
    """3 frames 2^31 + delta apart: separate eye buffers more than 4 GiB apart on the vector-eligible layout (the far base as
    well), side by side on the byte path."""
    k = FAMILIES.index(family)
    W, H = _size(True, k)
    _, lanes = _render(mods, orc, monkeypatch, slab, family, fp.Far(slab, "stride", apart=("right_",)), True, W, H, 3, False, 1000 + k)
    left, right = [a for a in lanes if a.name.split()[1] == "left_rgb"][0], [a for a in lanes if a.name.split()[1] == "right_rgb"][0]
    assert right.ptr - left.ptr > 1 << 32
    W, H = _size(False, k)
    _render(mods, orc, monkeypatch, slab, family, fp.Far(slab, "stride"), False, W, H, 3, True, 1100 + k)


@pytest.mark.parametrize("family", FAMILIES)
def test_render_batch_far_pitch(mods, orc, monkeypatch, slab, family):
    """Rows 2^29 + delta apart: two frames of 9 rows behind each other side by side on the vector-eligible layout, one frame of 11
    rows in separate eye buffers on the byte path."""
    k = FAMILIES.index(family)
    _render(mods, orc, monkeypatch, slab, family, fp.Far(slab, "pitch"), True, _size(True, k)[0], 9, 2, True, 1200 + k)
    _render(mods, orc, monkeypatch, slab, family, fp.Far(slab, "pitch"), False, _size(False, k)[0], 11, 1, False, 1300 + k)


@pytest.mark.parametrize("family", FAMILIES)
def test_render_single_far_pitch(mods, orc, monkeypatch, slab, family):
    """mdvt_render_stereo: one frame, rows 2^29 + delta apart."""
    k = FAMILIES.index(family)
    vec = bool(k % 2)
    W, H = _size(vec, k // 2)
    _render(mods, orc, monkeypatch, slab, family, fp.Far(slab, "pitch"), vec, W, H, 1, bool(k % 3 == 0), 1400 + k, single=True)


def test_render_null_byte_masks_far_stride(mods, orc, monkeypatch, slab):
    """The fused compaction without byte masks (test_render_null_byte_masks' case), with and without depth planes."""
    for k, want in enumerate((("bits", "counts", "depth"), ("bits", "counts"))):
        _render(mods, orc, monkeypatch, slab, "points_fast", fp.Far(slab, "stride", apart=("right_",) if k else ()), True, (64, 36)[k], (11, 9)[k],
                3, not k, 1500 + k, want=want)


@pytest.mark.parametrize("family,W,H,vec", [("points_general", 37, 11, False), ("mesh_general", 64, 64, True)])
def test_render_two_banks_far_stride(mods, orc, monkeypatch, slab, family, W, H, vec):
    """9 posed frames in launch sets of 4 on a workspace budget of 1 MiB (test_render_long_batches_on_two_banks' case: the sets take
    turns on two halves of the workspace and two streams), a quarter of 2^32 + delta apart: frame 2 lies past 2^31, frame 4 past 2^32."""
    far = fp.Far(slab, "stride", stride_unit=1 << 30)
    N = 9
    rng = np.random.default_rng(5)
    probe = tgf.RenderCase(mods, family, rng, fp.Layouts(rng, (0, 0, 0)), W, H, 1, sbs=False, ws_mib=1, kinds=[2])
    chunk = tgf._two_bank_sets(probe)
    probe.close()
    assert 2 <= chunk < N, (family, W, H, chunk)
    _, lanes = _render(mods, orc, monkeypatch, slab, family, far, vec, W, H, N, not vec, 1600 + W, want=("mask", "depth"), ws_mib=1, kinds=[2] * N)
    rgb = [a for a in lanes if "rgb" in a.name.split()[1] and a.input is None][0]
    assert 2 * rgb.stride > 1 << 31 and 4 * rgb.stride > 1 << 32 and rgb.n_frames == N


# --------------------------------------------------------------------------------------------- the stand-alone entry points
def _far_sweep(layouts):
    def sweep(n_random, seed):
        rng = np.random.default_rng(20261017 + seed)
        for vec in layouts:
            yield rng, _lays(rng, vec)
    return sweep


def _far_sizes(heights):
    def size(rng, *a, **kw):
        return int(rng.choice((36, 64) if size.vec else (33, 37))), int(rng.choice(heights))
    size.vec = False
    return size


def _run_family(monkeypatch, test, args, far, layouts, heights, entry, accepted):
    """One of tests/test_gpu_footprint.py's entry-point tests on far arenas: its sweep replaced by `layouts` (True: vector-eligible),
    its sizes by this file's.  -> the block's tally of the entry point."""
    monkeypatch.setattr(fp, "layout_sweep", _far_sweep(layouts))
    monkeypatch.setattr(tgf, "_size", _far_sizes(heights))
    with fp.far(far):
        test(*args)
        t = dict(fp.tally(entry))
    assert t["accepted"] >= accepted and t["odd_base"] >= 1 and t["padded"] >= accepted, (entry, t)
    return t


# name: (test of test_gpu_footprint.py, takes the oracle, the buffers whose pitch goes far (None: all))
SINGLE = {
    "mdvt_decode_depth": ("test_decode_depth", True, None),
    "mdvt_encode_depth": ("test_encode_depth", True, None),
    "mdvt_touchly_depth": ("test_touchly_depth", False, None),
    "mdvt_masked_blur": ("test_masked_blur", True, None),
    "mdvt_edge_filter": ("test_edge_filter", True, None),
    "mdvt_edge_point_pixels": ("test_edge_point_pixels", True, ("depth_rgb",)),        # (d_px is a tight array without a pitch)
    # include/mdvt.h: the plane a march walks keeps pitch < 2^24 and pitch x height < 2^32 (test_march_plane_limits); the other
    # buffers of the call go far
    "mdvt_infill_using_normals": ("test_infill_using_normals", True, ("color", "normal", "out")),
    "mdvt_mark_lower_side": ("test_mark_lower_side", True, ("out",)),
}


@pytest.mark.parametrize("entry", sorted(SINGLE))
def test_single_image_far_pitch(mods, orc, monkeypatch, slab, entry):
    name, with_orc, only = SINGLE[entry]
    _run_family(monkeypatch, getattr(tgf, name), (mods, orc) if with_orc else (mods,), fp.Far(slab, "pitch", only=only), (False, True), (9, 11),
                entry, 2)


# name: (test, takes the oracle, buffers whose pitch goes far, right-eye buffers of the far base)
BATCHED = {
    "mdvt_equirect_remap": ("test_equirect_remap", True, None, ()),
    "mdvt_swap_rb": ("test_swap_rb", False, None, ()),
    "mdvt_finish_infill_mask": ("test_finish_infill_mask", True, None, ()),
    "mdvt_finish_infill_mask_stereo": ("test_finish_infill_mask_stereo", True, None, ("seed_right", "out_right")),
    "mdvt_finish_infill_mask_heap": ("test_finish_infill_mask_heap", True, None, ()),
    "mdvt_finish_infill_mask_heap_stereo": ("test_finish_infill_mask_heap_stereo", True, None, ("seed_right", "out_right")),
    "mdvt_normal_infill": ("test_normal_infill", True, ("img", "out"), ()),
    "mdvt_infill_using_mask_normals": ("test_infill_using_mask_normals", True, ("img", "mask_img"), ()),
}


@pytest.mark.parametrize("entry", sorted(BATCHED))
def test_batched_far_stride(mods, orc, monkeypatch, slab, entry):
    """1, 2 and 3 images 2^31 + delta apart, on the byte path and on the vector-eligible layout (the sweep's cases take 1 + k % 3
    images: the six layouts put 3 images on either path); the right eye's buffers more than 4 GiB behind the left's."""
    name, with_orc, _, apart = BATCHED[entry]
    _run_family(monkeypatch, getattr(tgf, name), (mods, orc) if with_orc else (mods,), fp.Far(slab, "stride", apart=apart),
                (False, True, False, True, False, True), (9, 11), entry, 6)


@pytest.mark.parametrize("entry", sorted(BATCHED))
@pytest.mark.parametrize("first", ["bytes", "vector"])
def test_batched_far_pitch(mods, orc, monkeypatch, slab, entry, first):
    """Rows 2^29 + delta apart: one image and two images behind each other (9 rows: what the slab holds), either path first."""
    name, with_orc, only, _ = BATCHED[entry]
    _run_family(monkeypatch, getattr(tgf, name), (mods, orc) if with_orc else (mods,), fp.Far(slab, "pitch", only=only),
                (False, True) if first == "bytes" else (True, False), (9,), entry, 2)


def _march_case(mods, orc, entry, W, H, rng):
    """-> (body(run) -> status, check(out)) of one call of a march entry point; the far layout decides the pitches."""
    _lib, sr, _ = mods
    L = _lib.load()
    r = tgf._ctx(mods, W, H)
    if entry == "mdvt_infill_using_normals":
        color, hole, normal = tgf._march_scene(rng, W, H)

        def body(run):
            c, h = run.inp("color", color.reshape(1, H, 3 * W)), run.inp("hole", hole[None])
            n, o = run.inp("normal", normal.reshape(1, H, 3 * W)), run.out("out", H, 3 * W)
            return L.mdvt_infill_using_normals(r.ctx.handle, _vp(c), c.pitch, _vp(h), h.pitch, _vp(n), n.pitch, _vp(o), o.pitch, 400, tgf._stream())
        want = {"out": lambda: orc.infill_using_normals(color, hole.astype(bool), normal)}
    elif entry == "mdvt_mark_lower_side":
        _, img = tgf._ni_scene(rng, W, H)

        def body(run):
            a, o = run.inp("img", img.reshape(1, H, 3 * W)), run.out("out", H, 3 * W)
            return L.mdvt_mark_lower_side(r.ctx.handle, _vp(a), a.pitch, _vp(o), o.pitch, 30, tgf._stream())
        want = {"out": lambda: orc.mark_lower_side(img, 30)}
    elif entry == "mdvt_normal_infill":
        img, mask = tgf._ni_scene(rng, W, H)

        def body(run):
            a, m, o = run.inp("img", img.reshape(1, H, 3 * W)), run.inp("mask", mask.reshape(1, H, 3 * W)), run.out("out", H, 3 * W)
            return L.mdvt_normal_infill(r.ctx.handle, _vp(a), a.pitch, a.stride, _vp(m), m.pitch, m.stride, _vp(o), o.pitch, o.stride, 1, tgf._stream())
        want = {"out": lambda: orc.normal_infill(img, mask)}
    else:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        hole = tgf._march_scene(rng, W, H)[1]
        mimg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)

        def body(run):
            a, h = run.inp("img", img.reshape(1, H, 3 * W), inout=True), run.inp("hole", hole[None])
            m = run.inp("mask_img", mimg.reshape(1, H, 3 * W))
            return L.mdvt_infill_using_mask_normals(r.ctx.handle, _vp(a), a.pitch, a.stride, _vp(h), h.pitch, h.stride, _vp(m), m.pitch, m.stride, 1,
                                                    400, tgf._stream())
        want = {"img": lambda: orc.infill_using_normals(img, hole.astype(bool), ((mimg.astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32))}
    return r, body, want


# the plane each march walks with 32-bit offsets (mdvt_api.hip's guards; include/mdvt.h at mdvt_normal_infill)
MARCH_PLANE = {"mdvt_infill_using_normals": "hole", "mdvt_mark_lower_side": "img", "mdvt_normal_infill": "mask",
               "mdvt_infill_using_mask_normals": "hole"}


@pytest.mark.parametrize("entry", sorted(MARCH_PLANE))
def test_march_plane_limits(mods, orc, slab, entry):
    """include/mdvt.h: "pitches below 2^24 bytes and pitch x height below 2^32 (MDVT_ERR_UNSUPPORTED otherwise)".  The last accepted
    pitch, 2^24 - 1, gives the oracle's bytes, at 11 rows and at 256 rows (pitch x height = 2^32 - 256); the first refused pitch,
    2^24, and the first refused height at the last accepted pitch, 257, are refused with nothing touched."""
    plane = MARCH_PLANE[entry]
    for W, H, pitch, status in ((33, 11, (1 << 24) - 1, 0), (33, 11, 1 << 24, UNSUPPORTED), (37, 256, (1 << 24) - 1, 0), (37, 257, (1 << 24) - 1, UNSUPPORTED),
                                (33, 9, fp.FAR_PITCH + 9001, UNSUPPORTED)):
        assert (pitch < 1 << 24 and pitch * H <= 0xFFFFFFFF) == (status == 0)
        r, body, want = _march_case(mods, orc, entry, W, H, np.random.default_rng(W + H))
        try:
            with fp.far(fp.Far(slab, "pitch", only=(plane,), pitch=pitch, refusal=bool(status))):
                if status:
                    fp.refused(entry, body, status, seed=H)
                    continue

                def accepted(run):
                    r.ctx.check(body(run))
                out = fp.twice(entry, accepted, seed=H, what=f"{W}x{H} pitch {pitch} of '{plane}'")
                assert [a.pitch for a in fp.LAST_RUN if a.name.split()[1] == plane] == [pitch]
            for name, ref in want.items():
                assert np.array_equal(out[name].reshape(H, W, 3), ref()), (entry, W, H, pitch, name)
        finally:
            r.close()


# ------------------------------------------------------------------------------------------------------ convergence depths
@pytest.mark.parametrize("which", ["depth stride", "mask stride", "both strides", "both pitches", "depth pitch"])
def test_convergence_depths_far(mods, slab, which):
    """mdvt_convergence_depths: 3 depth frames and 2 mask frames (n_mask_frames < n_frames), the depth and the mask video far
    independently, both pixel orders, on the byte path and with the 12-byte loads' alignment."""
    _lib = mods[0]
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    kind = "stride" if "stride" in which else "pitch"
    only = None if "both" in which else (which.split()[0],)
    try:
        for k, vec in enumerate((False, True)):
            rng = np.random.default_rng(90 + k)
            W, H = _size(vec, k, heights=(9,))
            N, M = (3, 2) if kind == "stride" else (2, 1)
            order = k % 2
            depth = cr.random_depth(rng, N, H, W)
            mask = np.repeat(rng.choice(np.array([0, 240, 241, 255], np.uint8), (M, H, W, 1)), 3, axis=3)
            want, n = cr.clip_means(depth, mask)
            lays = _lays(rng, vec)
            ld, lm = lays.u8(), lays.u8()

            def body(run):
                d = run.inp("depth", (depth[..., ::-1] if order else depth).reshape(N, H, 3 * W), ld)
                m = run.inp("mask", (mask[..., ::-1] if order else mask).reshape(M, H, 3 * W), lm)
                o, c = run.out("means", 1, 4 * N, 1, fp.Layout(4 * k)), run.out("counts", 1, 4 * N, 1, fp.Layout(8))
                ctx.check(L.mdvt_convergence_depths(ctx.handle, W, H, _vp(d), d.pitch, d.stride, order, _vp(m), m.pitch, m.stride, order, N, M, 100.0,
                                                    _vp(o), _vp(c), None))
                far = [a for a in (d, m) if (a.stride > 1 << 31 if kind == "stride" else a.pitch > 1 << 29)]
                assert len(far) == (2 if only is None else 1) and (only is None or far[0] is run.arenas[only[0]])
            tag = f"{which}: {W}x{H} x{N}, {M} mask frames, order {order}, {ld}"
            with fp.far(fp.Far(slab, kind, only=only)):
                out = fp.twice("mdvt_convergence_depths", body, seed=k, what=tag)
            got = np.ascontiguousarray(out["means"]).view(np.float32).reshape(N)
            assert cr.same_bits(got, want).size == 0, f"{tag}: {got} vs {want}"
            assert np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(N).tolist() == n.tolist(), tag
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------- FFV1
def _video_frames(rng, N, H, W):
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    for f in range(N):
        frames[f, :, : W // 2] = 40 + f                                       # a flat half: short packets, each frame its own
    return frames


@pytest.mark.parametrize("vec", [False, True])
def test_encode_video_frames_far_stride(mods, slab, vec):
    """3 source frames 2^31 + delta apart: every packet is byte for byte mdvt_ffv1_encode_frame's."""
    _lib = mods[0]
    from metric_depth_video_toolbox_amd import ffv1_device as fd, video_io
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        rng = np.random.default_rng(70 + vec)
        W, H = _size(vec, int(vec))
        N, slices, bgr = 3, (2, 2), int(vec)
        frames = _video_frames(rng, N, H, W)
        host = [video_io.encode_frame(f, slices=slices, bgr=bool(bgr), threads=1)[0] for f in frames]
        cap = N * fd.packet_capacity_bytes(W, H, slices, 0)
        li = _lays(rng, vec).u8()
        res = []
        with fp.far(fp.Far(slab, "stride")):
            for comp in (False, True):
                run = fp.new_run("mdvt_encode_video_frames", comp, 7, "cuda")
                a = run.inp("src", frames.reshape(N, H, 3 * W), li)
                p, o, s = run.out("packets", 1, cap), run.out("offsets", 1, 8 * N), run.out("sizes", 1, 4 * N)
                assert a.stride > 1 << 31
                ctx.check(L.mdvt_encode_video_frames(ctx.handle, W, H, slices[0], slices[1], _vp(a), a.pitch, a.stride, 3, bgr, N, 0, _vp(p), cap,
                                                     _vp(o), _vp(s), tgf._stream()))
                out = run.check()
                sizes = np.ascontiguousarray(out["sizes"]).view(np.uint32).reshape(-1)
                offs = np.ascontiguousarray(out["offsets"]).view(np.uint64).reshape(-1)
                assert all(int(v) < fd.TOO_LARGE for v in sizes) and int(offs[-1]) + int(sizes[-1]) <= cap
                res.append([out["packets"].reshape(-1)[int(offs[f]):int(offs[f]) + int(sizes[f])].tobytes() for f in range(N)])
        assert res[0] == res[1] == host
    finally:
        ctx.close()


@pytest.mark.parametrize("vec", [False, True])
def test_decode_video_frames_far(mods, slab, vec):
    """Packets 2^31 + delta apart inside d_packets (d_offsets[1] past 2^31, d_offsets[2] past 2^32, packets_bytes to match) into
    frames 2^31 + delta apart.  Then packets_bytes one byte short of the last packet's end: MDVT_FFV1_BAD_PACKET for that frame
    only, the others decoded."""
    _lib = mods[0]
    from metric_depth_video_toolbox_amd import video_io
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)
    try:
        rng = np.random.default_rng(80 + vec)
        W, H = _size(vec, int(vec))
        N, slices, order = 3, (2, 2), int(vec)
        frames = _video_frames(rng, N, H, W)
        pk = [video_io.encode_frame(f, slices=slices) for f in frames]
        packets, cfg = [x[0] for x in pk], pk[0][1]
        longest = max(len(p) for p in packets)
        sizes = np.array([len(p) for p in packets], np.uint32)
        ld = _lays(rng, vec).u8()
        for short in (0, 1):
            def body(run):
                # the packet buffer as a lane of 3 "frames" of one row: packet k at k * stride, poison behind each packet's end
                blob = run.out("blob", 1, longest, N, fp.Layout(ld.base, 0, 0))
                host = blob.poison.copy()
                for f in range(N):
                    host[blob.pay_index[f, 0, :len(packets[f])]] = np.frombuffer(packets[f], np.uint8)
                slab.put(blob.iv_start, blob.iv_len, host)
                blob.input = host[blob.pay_index].copy()
                offs = np.arange(N, dtype=np.uint64) * np.uint64(blob.stride)
                assert offs[1] > 1 << 31 and offs[2] > 1 << 32
                total = int(offs[-1]) + len(packets[-1]) - short
                o = run.inp("offsets", offs.view(np.uint8).reshape(1, 1, -1), fp.Layout(8))
                s = run.inp("sizes", sizes.view(np.uint8).reshape(1, 1, -1))
                d, st = run.out("dst", H, 3 * W, N, ld), run.out("status", 1, 4 * N)
                assert d.stride > 1 << 31
                ctx.check(L.mdvt_decode_video_frames(ctx.handle, W, H, cfg, len(cfg), _vp(blob), total, _vp(o), _vp(s), N, _vp(d), d.pitch, d.stride,
                                                     order, _vp(st), None))
            with fp.far(fp.Far(slab, "stride")):
                if not short:
                    out = fp.twice("mdvt_decode_video_frames", body, seed=3, what=f"{W}x{H} x{N}")
                else:                                               # (a flagged frame's bytes are unspecified inside its own rows)
                    run = fp.new_run("mdvt_decode_video_frames", False, 3, "cuda")
                    body(run)
                    out = run.check()
            status = np.ascontiguousarray(out["status"]).view(np.uint32).reshape(N).tolist()
            assert status == [0, 0, 4 if short else 0], status
            want = frames[..., ::-1] if order else frames
            assert np.array_equal(out["dst"].reshape(N, H, W, 3)[:N - short], want[:N - short])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------- library-owned blocks past 4 GiB
def test_encoder_scratch_block_past_4_gib(mods, slab):
    """The device encoder's scratch is slices x slice_stride: 20 frames of 64 x 64 in 4 x 4 slices with slice_capacity 2^24 - 1 and
    a workspace budget of 8 GiB make it 20 x 16 x 2^24 bytes = 5 GiB, one pass.  Every packet equals the host encoder's."""
    _lib = mods[0]
    from metric_depth_video_toolbox_amd import ffv1_device as fd, video_io
    L = _lib.load()
    W = H = 64
    N, slices, cap24 = 20, (4, 4), (1 << 24) - 1
    assert N * 16 * (cap24 + 8) > 1 << 32
    r = tgf._ctx(mods, W, H, workspace_mib=8192)
    ctx = r.ctx
    try:
        rng = np.random.default_rng(77)
        frames = _video_frames(rng, N, H, W)
        host = [video_io.encode_frame(f, slices=slices, threads=1)[0] for f in frames]
        src = torch.from_numpy(frames).cuda()
        room = N * fd.packet_capacity_bytes(W, H, slices, 0)
        pk = torch.zeros(room, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(N, dtype=torch.int64, device="cuda")
        sizes = torch.zeros(N, dtype=torch.int32, device="cuda")
        ctx.check(L.mdvt_encode_video_frames(ctx.handle, W, H, 4, 4, C.c_void_p(src.data_ptr()), 3 * W, 3 * W * H, 3, 0, N, cap24,
                                             C.c_void_p(pk.data_ptr()), room, C.c_void_p(offs.data_ptr()), C.c_void_p(sizes.data_ptr()), tgf._stream()))
        torch.cuda.synchronize()
        assert ctx.workspace_bytes() >= 1 << 32, f"the scratch block stayed below 4 GiB ({ctx.workspace_bytes()} bytes): the pass took fewer than {N} frames"
        pk, offs, sizes = pk.cpu().numpy(), offs.cpu().numpy(), sizes.cpu().numpy().view(np.uint32)
        for f in range(N):
            assert int(sizes[f]) == len(host[f]) and pk[int(offs[f]):int(offs[f]) + int(sizes[f])].tobytes() == host[f], f
    finally:
        r.close()
        L.mdvt_release_cached_memory(-1)


def test_heap_completion_workspace_past_4_gib(mods, orc, slab):
    """The heap-order completion keeps n_images x 44 B/px in one block addressed as ws + im x image_bytes: 256 images of 832 x 480
    are 4.5 GB.  Three distinct seed images sit at the first slot, the last, and the slots on either side of 2^31 and of 2^32; the
    rest are copies.  Every slot equals its image's reference (one oracle run per distinct image)."""
    _lib, sr, _ = mods
    L = _lib.load()
    W, H, N = 832, 480, 256
    rng = np.random.default_rng(44)
    base = []
    for _ in range(3):
        s = np.zeros((H, W, 3), np.uint8)
        s[rng.integers(0, 256, (H, W)) < 250] = (90, 160, 200)                         # known almost everywhere: small holes
        s[..., 0] += rng.integers(0, 40, (H, W), dtype=np.uint8)
        for _ in range(12):
            x0, y0 = int(rng.integers(4, W - 12)), int(rng.integers(4, H - 12))
            s[y0:y0 + int(rng.integers(2, 7)), x0:x0 + int(rng.integers(2, 7))] = tgf.GREEN
        base.append(s)
    r = tgf._ctx(mods, W, H, infill_mask=True)
    try:
        seeds = torch.from_numpy(base[0]).cuda()[None].repeat(N, 1, 1, 1)
        which = np.zeros(N, np.int64)
        # mdvt_telea_heap.hip's telea_heap_image_bytes, restated: planes of 8 + 8 x 4 + 3 (+ 4 bytes) + 1 bytes per pixel, each
        # rounded up to 256 bytes
        plane = lambda n: (n + 255) & ~255
        per = plane(8 * W * H) + 8 * plane(4 * W * H) + plane(3 * W * H + 4) + plane(W * H)
        assert N * per > 1 << 32
        for bound, img in ((1 << 31, 1), (1 << 32, 2)):
            lo = bound // per                                  # slot lo begins below the boundary, slot lo + 1 above
            assert lo * per < bound < (lo + 1) * per and lo + 1 < N - 1
            which[lo] = which[lo + 1] = img
        which[N - 1] = 2
        for sl in np.flatnonzero(which):
            seeds[sl] = torch.from_numpy(base[which[sl]]).cuda()
        out = torch.zeros_like(seeds)
        rem = torch.full((N,), 0x55, dtype=torch.int32, device="cuda")
        r.ctx.check(L.mdvt_finish_infill_mask_heap(r.ctx.handle, C.c_void_p(seeds.data_ptr()), 3 * W, 3 * W * H, C.c_void_p(out.data_ptr()), 3 * W,
                                                   3 * W * H, N, C.c_void_p(rem.data_ptr()), tgf._stream()))
        torch.cuda.synchronize()
        ws = r.ctx.workspace_bytes()
        assert ws >= 1 << 32, f"the pass took fewer than {N} images: the context holds {ws} bytes of workspace, less than 2^32"
        refs = [tgf._fmm_finish(orc, b) for b in base]
        got, rem = out.cpu().numpy(), rem.cpu().numpy().view(np.uint32)
        for sl in range(N):
            want, wrem = refs[which[sl]]
            assert np.array_equal(got[sl], want), f"slot {sl} (image {which[sl]})"
            assert int(rem[sl]) == wrem, (sl, int(rem[sl]), wrem)
    finally:
        r.close()
        L.mdvt_release_cached_memory(-1)
