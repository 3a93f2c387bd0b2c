"""Every entry point of include/mdvt.h that writes device memory, held to its footprint (tests/footprint.py): through the raw C ABI,
with every buffer inside a poisoned arena -- odd base offsets, padded pitches, padded strides, separate eye buffers -- each case
once on a pseudo-random poison and once on its complement:

  1. no byte outside an output's payload changes (guards, pitch padding, gaps between frames), and no input byte at all;
  2. every payload byte is equal in the two runs (so it was written, not accumulated into, and depends on nothing beyond an input);
  3. the payload equals the reference (the C oracle; NumPy for Touchly and the channel swap) -- every comparison is equality;
  4. layouts the header refuses are refused with the documented status and leave every arena as it was.

Each test prints its entry point's row: accepted / refused layouts, bytes of guard and padding checked."""
import ctypes as C

import numpy as np
import pytest

import footprint as fp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INVALID, UNSUPPORTED = -1, -3
IMIN = np.iinfo(np.int32).min
GREEN = (0, 255, 0)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import _lib, stereo_rerender, synthetic
    return _lib, stereo_rerender, synthetic


def _K(p):
    return np.array([p.K[k] for k in range(9)]).reshape(3, 3)


def _vp(a):
    return C.c_void_p(a if isinstance(a, int) else a.ptr)


def _code_to_rgb(code):
    code = np.minimum(code, 65535).astype(np.uint32)
    d = np.zeros(code.shape + (3,), np.uint8)
    d[..., 0] = d[..., 1] = (code >> 8) & 0xFF
    d[..., 2] = code & 0xFF
    return d


def _depth_scene(rng, W, H, noise_ok=True):
    """RGB-coded depth with the structure of sweep_cases' styles; white noise only where the oracle can afford it."""
    style = int(rng.integers(4 if noise_ok and W * H <= 4096 else 3))
    if style == 0:                                       # foreground rectangles over a far plane, a patch of depth code 0
        code = np.full((H, W), int(rng.integers(3000, 60000)), np.uint32)
        for _ in range(int(rng.integers(1, 6))):
            x0, y0 = int(rng.integers(W)), int(rng.integers(H))
            code[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, max(2, W // 2)))] = int(rng.integers(50, 3000))
        if W > 8:
            code[0, 3:5] = 0
    elif style == 1:                                     # smooth plane + a step
        code = (2000 + 40 * np.arange(W)[None, :] + 7 * np.arange(H)[:, None]).astype(np.uint32)
        code[:, W // 2:] //= 3
    elif style == 2:                                     # one-code noise on a slope: ties and 1-LSB steps
        code = (int(rng.integers(300, 40000)) + np.arange(W)[None, :] // 3 + rng.integers(0, 2, (H, W))).astype(np.uint32)
    else:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return _code_to_rgb(code)


VEC_WIDTHS = (8, 12, 16, 32, 64, 128, 252, 256)


def _size(rng, min_w=1, min_h=1, wide=False, max_w=257):
    """A frame size from the issue's lists; for a vector-eligible layout (_size.vec, set per case by the sweeps) a width that is a
    multiple of 4, at least 8."""
    if _size.vec:
        if wide and _size.vec == "wide":                                          # (the sweeps' last vector-eligible layout)
            return int(rng.choice([w for w in fp.LDS_WIDTHS if w % 4 == 0])), int(rng.choice((2, 3)))
        return int(rng.choice([w for w in VEC_WIDTHS if w <= max_w])), int(rng.choice([h for h in fp.HEIGHTS if h >= max(min_h, 2)]))
    if wide and rng.integers(6) == 0:
        return int(rng.choice(fp.LDS_WIDTHS)), int(rng.choice((2, 3)))
    ws = [w for w in fp.WIDTHS if min_w <= w <= max_w]
    hs = [h for h in fp.HEIGHTS if h >= min_h]
    return int(rng.choice(ws)), int(rng.choice(hs))


_size.vec = False


def _io_vec4(io, W, zout):
    """plan.vec4 of mdvt_render_stereo_batch (mdvt_api.hip), restated: what sends a frame to the vector kernels -- k_mesh_band,
    k_mesh_conv, the vec4 point rows -- instead of the byte paths."""
    def al(v, a=4):
        return (v or 0) % a == 0
    ok = (W % 4 == 0 and al(io.depth_rgb) and al(io.color_rgb) and al(io.left_rgb) and al(io.right_rgb) and al(io.left_mask) and
          al(io.right_mask) and al(io.depth_pitch) and al(io.color_pitch) and al(io.rgb_pitch) and al(io.mask_pitch) and
          al(io.depth_stride) and al(io.color_stride) and al(io.rgb_stride) and al(io.mask_stride))
    if io.left_seed:
        ok = ok and al(io.left_seed) and al(io.right_seed) and al(io.seed_pitch) and al(io.seed_stride)
    if zout:
        ok = ok and al(io.left_depth, 16) and al(io.right_depth, 16) and al(io.zout_pitch, 16) and al(io.zout_stride, 16)
    return bool(ok)


FAMILY_VECTOR = {}                    # family -> accepted layouts on the vector path with a padded output pitch


# ------------------------------------------------------------------------------------------------------------------ render
FAMILIES = {
    # name: (renderer keywords, frame kinds it may draw (0 pure shift, 1 convergence, 2 pose, 3 both), optional outputs it supports)
    "points_fast": (dict(render_as_pointcloud=True), (0,), ("depth", "bits", "counts")),
    "points_fast_grid4": (dict(render_as_pointcloud=True, subpixel_bits=4), (0,), ("depth", "bits", "counts")),
    "points_general": (dict(render_as_pointcloud=True), (1, 2, 3), ("depth", "bits", "counts")),
    "points_edges1": (dict(render_as_pointcloud=True, infill_mask=True), (0, 0, 1, 2), ("depth", "bits", "counts", "seed")),
    "points_edges0": (dict(render_as_pointcloud=True, remove_edges=True, dont_place_points_in_edges=True), (0, 2), ("depth", "bits", "counts", "seed")),
    "mesh_band": (dict(), (0,), ("depth", "bits", "counts")),
    "mesh_band_grid4": (dict(subpixel_bits=4), (0,), ("depth", "bits", "counts")),
    "mesh_conv": (dict(), (1,), ("depth", "bits", "counts")),                  # MDVT_MESH_CONV=1 on the tuning library: k_mesh_conv
    "mesh_general": (dict(), (1, 2, 3), ("depth", "bits", "counts")),
    "mesh_edges1": (dict(infill_mask=True), (0, 0, 1, 2), ("depth", "bits", "counts", "seed")),
    "mesh_edges2": (dict(infill_mask=True, do_basic_infill=True), (0, 1, 3), ("depth", "bits", "counts", "seed")),
    "mesh_edges0": (dict(remove_edges=True, dont_place_points_in_edges=True), (0, 2), ("depth", "bits", "counts", "seed")),
    "mesh_msaa": (dict(samples=4), (0, 1, 2), ("counts",)),
    "points_msaa": (dict(render_as_pointcloud=True, samples=4, sample_pattern=1, sample_resolve=1), (0, 2), ("counts",)),
    "mesh_near_clip": (dict(near_clip=True), (0, 2), ("counts",)),
}


def _eye(out, name, e, row_bytes):
    """The payload of eye e: a column half of the side-by-side arena, or the eye's own arena."""
    if name in out:
        return out[name][:, :, e * row_bytes:(e + 1) * row_bytes]
    return out[("left_", "right_")[e] + name]


class RenderCase:
    def __init__(self, mods, family, rng, lays, W, H, N, sbs, kinds=None, ws_mib=0, force_batch=False, conv=None):
        self._lib, self.sr, synthetic = mods
        self.family, self.W, self.H, self.N, self.sbs = family, W, H, N, sbs
        kw, fam_kinds, self.optional = FAMILIES[family]
        self.kw = dict(kw)
        if ws_mib:
            self.kw["workspace_mib"] = ws_mib
        self.kinds = kinds if kinds is not None else [int(rng.choice(fam_kinds)) for _ in range(N)]
        self.entry = "mdvt_render_stereo" if N == 1 and not force_batch else "mdvt_render_stereo_batch"
        self.depth = np.stack([_depth_scene(rng, W, H, noise_ok=not family.endswith("msaa")) for _ in range(N)])
        self.color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        key = GREEN if self.kw.get("infill_mask") else (0, 0, 0)
        self.color[0, int(rng.integers(H)), int(rng.integers(W))] = key           # the colour-key rule inside the image
        track = synthetic.synthetic_pose_track(64)
        self.Ts = [track[int(rng.integers(1, 64))] if k >= 2 else None for k in self.kinds]
        self.convs = [float(rng.uniform(1.0 if family == "mesh_conv" else 0.5, 8.0)) if k in (1, 3) else None for k in self.kinds]
        if conv is not None:
            self.convs = [conv if k in (1, 3) else None for k in self.kinds]
        self.ipd = int(rng.choice([30, 63, 65, 120]))
        self.xfov = float(rng.choice([45.0, 60.0, 90.0]))
        self.lays = lays
        # one layout per buffer, drawn once: both poison runs and every optional-output variant use the same
        self.L = dict(d=lays.u8(), c=lays.u8(), rgb=lays.u8(), mask=lays.u8(), z=lays.w32(), bits=lays.w32(), seed=lays.u8(),
                      counts=fp.Layout(int(rng.choice(fp.BASES4)), 0, 0))
        self.base_r = dict(rgb=int(rng.choice(fp.BASES)), mask=int(rng.choice(fp.BASES)), z=int(rng.choice(fp.BASES4)),
                           bits=int(rng.choice(fp.BASES4)), seed=int(rng.choice(fp.BASES)))
        if lays.fixed is not None:
            self.base_r = {k: (lays.fixed[0] if k in ("rgb", "mask", "seed") else 0 if lays.vec else lays.fixed[0] & ~3) for k in self.base_r}
        self.r = self.sr.StereoRerenderer(W, H, pupillary_distance=self.ipd, **self.kw)
        self.ps = [self.r.frame_params(xfov=self.xfov, convergence_distance=self.convs[f], transformation=self.Ts[f]) for f in range(N)]
        self.rowb = 4 * ((W + 31) // 32)
        if family == "mesh_conv":
            # k_mesh_conv takes a converged frame whose vertex rows tilt by at most 12 rows across the frame (fill_frame_dev's
            # conv_band); an upper estimate of that tilt, kept below 10, so that the frames of this family really go to it
            for p in self.ps:
                sn, cs_, span = abs(np.sin(p.convergence_angle)), np.cos(p.convergence_angle), W / p.K[0]
                assert p.convergence_angle != 0 and sn * span * (H / 2 + 1) / (cs_ - sn * span) ** 2 <= 10, "toe-in too strong for k_mesh_conv"

    def tag(self):
        return (f"{self.family} {self.W}x{self.H} x{self.N} {'sbs' if self.sbs else 'separate eyes'} kinds={self.kinds} ipd={self.ipd} "
                f"xfov={self.xfov} layouts={self.L} right-eye bases={self.base_r}")

    def close(self):
        self.r.close()

    def predict_vec4(self, want):
        """plan.vec4 from the layouts alone (W % 4 == 0 makes every tight row a multiple of 4, every float row one of 16)."""
        use = [self.L["d"], self.L["c"], self.L["rgb"]] + [self.L[k] for k in ("mask", "seed") if k in want]
        rights = [] if self.sbs else [self.base_r[k] for k in ("rgb", "mask", "seed") if k == "rgb" or k in want]
        ok = self.W % 4 == 0 and all(l.base % 4 == 0 and l.pad % 4 == 0 and l.gap % 4 == 0 for l in use) and all(b % 4 == 0 for b in rights)
        if "depth" in want:
            z = self.L["z"]
            ok = ok and z.base % 16 == 0 and z.pad % 16 == 0 and z.gap % 16 == 0 and (self.sbs or self.base_r["z"] % 16 == 0)
        return bool(ok)

    def count(self):
        """Tally the case twice() just accepted; vector = the frames went to the family's vector kernel (plan.vec4, and a width the
        LDS row / band kernels take)."""
        vector = self.vec4 and 8 <= self.W <= 4096
        got = fp.accepted(self.entry, vector=vector)
        FAMILY_VECTOR[self.family] = FAMILY_VECTOR.get(self.family, 0) + int(got[2])
        return vector

    def _pair(self, run, name, row_bytes, lay_key, io, fl, fr, fp_, fs):
        """The output buffers of one kind for both eyes -> the io record's two pointers, pitch and stride."""
        H, N = self.H, self.N
        lay = self.L[lay_key]
        if self.sbs:
            a = run.out(name, H, 2 * row_bytes, N, lay)
            lp, rp, pitch, stride = a.ptr, a.ptr + row_bytes, a.pitch, a.stride
        else:
            a = run.out("left_" + name, H, row_bytes, N, lay)
            b = run.out("right_" + name, H, row_bytes, N, fp.Layout(self.base_r[lay_key], lay.pad, lay.gap))
            lp, rp, pitch, stride = a.ptr, b.ptr, a.pitch, a.stride
        setattr(io, fl, lp); setattr(io, fr, rp); setattr(io, fp_, pitch); setattr(io, fs, stride)

    def body(self, want, status=None, break_io=None):
        """-> body(run) for fp.twice / fp.refused.  want: the outputs requested besides the RGB images ("mask" among them)."""
        def run_body(run):
            W, H, N = self.W, self.H, self.N
            io = self._lib.MdvtIO()
            d = run.inp("depth_rgb", self.depth.reshape(N, H, 3 * W), self.L["d"])
            c = run.inp("color_rgb", self.color.reshape(N, H, 3 * W), self.L["c"])
            io.depth_rgb, io.depth_pitch, io.depth_stride = d.ptr, d.pitch, d.stride
            io.color_rgb, io.color_pitch, io.color_stride = c.ptr, c.pitch, c.stride
            self._pair(run, "rgb", 3 * W, "rgb", io, "left_rgb", "right_rgb", "rgb_pitch", "rgb_stride")
            if "mask" in want:
                self._pair(run, "mask", W, "mask", io, "left_mask", "right_mask", "mask_pitch", "mask_stride")
            if "depth" in want:
                self._pair(run, "depth", 4 * W, "z", io, "left_depth", "right_depth", "zout_pitch", "zout_stride")
            if "bits" in want:
                self._pair(run, "bits", self.rowb, "bits", io, "left_maskbits", "right_maskbits", "maskbits_pitch", "maskbits_stride")
            if "seed" in want:
                self._pair(run, "seed", 3 * W, "seed", io, "left_seed", "right_seed", "seed_pitch", "seed_stride")
            if "counts" in want:
                io.hole_counts = run.out("counts", 1, 8 * N, 1, self.L["counts"]).ptr
            if break_io:
                break_io(io)
            self.vec4 = _io_vec4(io, W, "depth" in want)
            Lb = self._lib.load()
            arr = (self._lib.MdvtFrameParams * N)(*self.ps)
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if self.entry == "mdvt_render_stereo":
                rc = Lb.mdvt_render_stereo(self.r.ctx.handle, C.byref(arr[0]), C.byref(io), s)
            else:
                rc = Lb.mdvt_render_stereo_batch(self.r.ctx.handle, N, arr, C.byref(io), s)
            if status is None:
                self.r.ctx.check(rc)
            return rc
        return run_body

    def reference(self, orc, f):
        r, p = self.r, self.ps[f]
        op = orc.make_params(self.W, self.H, _K(p), ipd_m=self.ipd / 1000, max_depth=r.max_depth, depth_scale=p.depth_scale,
                             mode=orc.MODE_POINTS if r.mode == 0 else orc.MODE_MESH, remove_edges=r.remove_edges,
                             edge_points=(2 if r.do_basic_infill else 1) if r.edge_points else 0, conv_angle=p.convergence_angle,
                             T=self.Ts[f], key_rgb=r.key_rgb, subpixel_bits=r.subpixel_bits)
        if r.samples == 4 or (r.near_clip and r.mode == 1):
            return orc.render_stereo_gl(op, self.depth[f], self.color[f], near_clip=r.near_clip and r.mode == 1, samples=r.samples,
                                        pattern=r.sample_pattern, resolve=r.sample_resolve)
        return orc.render_stereo(op, self.depth[f], self.color[f], want_depth=True, want_seed=r.remove_edges)

    def compare(self, out, wants, want, tag):
        """Property 3 on the outputs requested; wants: the reference per frame."""
        W, H, N = self.W, self.H, self.N
        for f in range(N):
            w = wants[f]
            for e, eye in enumerate(("left", "right")):
                t = f"{tag}: frame {f} {eye}"
                assert np.array_equal(_eye(out, "rgb", e, 3 * W)[f].reshape(H, W, 3), w[eye + "_rgb"]), t + " rgb"
                hole = w[eye + "_mask"] > 0
                if "mask" in want:
                    assert np.array_equal(_eye(out, "mask", e, W)[f], w[eye + "_mask"]), t + " mask"
                if "depth" in want:
                    z = np.ascontiguousarray(_eye(out, "depth", e, 4 * W)[f]).view(np.uint32)
                    assert np.array_equal(z, w[eye + "_depth"].view(np.uint32)), t + " depth plane"
                if "bits" in want:
                    # include/mdvt.h: the rows are padded to whole dwords and the call owns them; bits beyond W are zero
                    pk = np.zeros((H, self.rowb), np.uint8)
                    pb = np.packbits(hole, axis=1, bitorder="little")
                    pk[:, :pb.shape[1]] = pb
                    assert np.array_equal(_eye(out, "bits", e, self.rowb)[f], pk), t + " packed mask (bits beyond W must be zero)"
                if "counts" in want:
                    cnt = np.ascontiguousarray(out["counts"]).view(np.uint32).reshape(-1)
                    assert int(cnt[2 * f + e]) == int(hole.sum()), t + f" hole count {int(cnt[2 * f + e])} != {int(hole.sum())}"
                if "seed" in want:
                    assert np.array_equal(_eye(out, "seed", e, 3 * W)[f].reshape(H, W, 3), w[eye + "_seed"]), t + " seed image"


def _render_sweep(mods, orc, monkeypatch, family, n_random, seed, batches=(1,), wide=False):
    """One family's layouts x sizes: all outputs requested on every case; on the first, also none and each optional output alone."""
    if family == "mesh_conv":
        monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")
        monkeypatch.setenv("MDVT_MESH_CONV", "1")
    edges = FAMILIES[family][0].get("infill_mask") or FAMILIES[family][0].get("remove_edges")
    for k, (rng, lays) in enumerate(fp.layout_sweep(n_random, seed)):
        _size.vec = "wide" if lays.vec and k == fp.FIRST_VEC + len(fp.VEC_FIXED) - 1 else lays.vec
        W, H = _size(rng, 3 if edges else 2, 3 if edges else 2, wide=wide)
        _size.vec = False
        N = int(batches[k % len(batches)])
        ws_mib = 0
        if N > 3:                                        # short launch sets on two banks, as batch_sweep_cases gets them
            ws_mib = max(1, -(-2 * W * H * (16 + 48 + 32 + 24 + 3) // (1 << 20)))
        cs = RenderCase(mods, family, rng, lays, W, H, N, sbs=bool(k % 3 == 2) and not lays.vec, ws_mib=ws_mib,
                        force_batch=(N == 1 and k % 2 == 1 and len(batches) > 1))
        optional = cs.optional
        full = ("mask",) + optional
        tag = cs.tag()
        try:
            out = fp.twice(cs.entry, cs.body(full), seed=seed * 100 + k, what=tag)
            wants = [cs.reference(orc, f) for f in range(N)]
            cs.compare(out, wants, full, tag)
            cs.count()
            assert cs.vec4 or not lays.vec, f"{tag}: a layout made for the vector path does not meet plan.vec4"
            if k in (0, fp.FIRST_ODD, fp.FIRST_VEC):          # tight; odd base and padded; vector path, padded, gaps
                for sub in [("mask",)] + [("mask", o) for o in optional]:
                    o2 = fp.twice(cs.entry, cs.body(sub), seed=seed * 100 + k, what=f"{tag} outputs={sub}")
                    cs.compare(o2, wants, sub, f"{tag} outputs={sub}")
                    for name in o2:
                        assert np.array_equal(o2[name], out[name]), f"{tag}: '{name}' differs when only {sub} is requested"
                    cs.count()
            # layouts the header refuses: a packed mask whose rows are not dword aligned, a pitch shorter than a row
            if "bits" in optional and k % 4 == 0:
                def misaligned(io, k=k):
                    if k % 8 == 0:
                        io.maskbits_pitch += 2
                    else:
                        io.left_maskbits += 2
                fp.refused(cs.entry, cs.body(full, status=INVALID, break_io=misaligned), INVALID, seed=k)
            if k % 4 == 1:
                def short_pitch(io, k=k, W=W):
                    if k % 8 == 1:
                        io.rgb_pitch = 3 * W - 1
                    else:
                        io.mask_pitch = W - 1
                fp.refused(cs.entry, cs.body(full, status=INVALID, break_io=short_pitch), INVALID, seed=k)
            if ("msaa" in family or "near" in family) and k % 4 == 2:
                fp.refused(cs.entry, cs.body(("mask", "depth"), status=UNSUPPORTED), UNSUPPORTED, seed=k)
        finally:
            cs.close()
    assert FAMILY_VECTOR.get(family, 0) >= 1, f"{family}: no accepted layout reached the vector kernels (plan.vec4) with a padded pitch"


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_render_single_frames(mods, orc, monkeypatch, family):
    """"mdvt_render_stereo" in every kernel family, on the layout sweep and on widths around the LDS limits."""
    wide = family in ("points_fast", "mesh_band", "mesh_edges1", "points_edges1", "points_general")
    _render_sweep(mods, orc, monkeypatch, family, 6 if "msaa" in family else 10, seed=11 + sorted(FAMILIES).index(family), wide=wide)
    fp.finish_entry("mdvt_render_stereo", need_vector=True)


@pytest.mark.parametrize("family", ["points_fast", "points_general", "points_edges1", "mesh_band", "mesh_conv", "mesh_general", "mesh_edges1",
                                    "mesh_msaa", "mesh_near_clip"])
def test_render_batches(mods, orc, monkeypatch, family):
    """"mdvt_render_stereo_batch": 1, 2, 3 frames and one batch long enough for two banks of launch sets; frames of mixed kinds
    where the family has several."""
    _render_sweep(mods, orc, monkeypatch, family, 3, seed=101 + sorted(FAMILIES).index(family), batches=(2, 3, 1, 9 if "msaa" not in family else 4))
    fp.finish_entry("mdvt_render_stereo_batch", need_vector=True)


def test_render_mixed_kinds_in_one_batch(mods, orc):
    """Pure-shift, converged and posed frames in one call: every run of frames has its own launches and its own part of the arenas."""
    for family in ("points_edges1", "mesh_edges1"):
        for k, (rng, lays) in enumerate(fp.layout_sweep(2, 301)):
            if k % 3:
                continue
            _size.vec = lays.vec
            W, H = _size(rng, 3, 3)
            _size.vec = False
            cs = RenderCase(mods, family, rng, lays, W, H, 7, sbs=bool(k % 2), kinds=[0, 1, 1, 0, 2, 3, 0])
            full = ("mask",) + cs.optional
            try:
                out = fp.twice(cs.entry, cs.body(full), seed=300 + k, what=cs.tag())
                cs.compare(out, [cs.reference(orc, f) for f in range(7)], full, cs.tag())
                cs.count()
            finally:
                cs.close()
    fp.finish_entry("mdvt_render_stereo_batch", need_odd=False, need_padded=False)


def test_render_null_byte_masks(mods, orc):
    """ABI 0.15: no byte masks, the packed mask alone, where the compaction is fused into the point kernel (pure shift, no edge
    removal, W % 4 == 0, W <= 4096, dword-aligned images: include/mdvt.h); every other width or layout is refused and nothing is
    touched."""
    ran = ran_z = ran_padded = 0
    for k, (rng, lays) in enumerate(fp.layout_sweep(6, 401)):
        _size.vec = lays.vec
        W, H = _size(rng, 2, 2, wide=True)
        _size.vec = False
        if k < 8:
            W = (4, 8, 16, 32, 64, 128, 252, 256)[k]
        cs = RenderCase(mods, "points_fast", rng, lays, W, H, 1 + k % 3, sbs=bool(k % 2))
        want = ("bits", "counts", "depth") if k % 2 == 0 else ("bits", "counts")       # the depth planes want 16-byte alignment
        try:
            if W <= 4096 and cs.predict_vec4(want):
                tag = cs.tag() + f" NULL byte masks, outputs={want}"
                out = fp.twice(cs.entry, cs.body(want), seed=400 + k, what=tag)
                assert cs.vec4, tag + ": the layout's prediction and the call's own pointers disagree about plan.vec4"
                cs.compare(out, [cs.reference(orc, f) for f in range(cs.N)], want, tag)
                ran_padded += int(cs.count() and cs.L["rgb"].pad > 0)
                ran += 1
                ran_z += int("depth" in want)
            else:
                fp.refused(cs.entry, cs.body(want, status=INVALID), INVALID, seed=k)
                if W % 4 == 0 and W <= 4096 and k % 2 == 0 and cs.predict_vec4(("bits", "counts")):
                    # refused for the depth planes' alignment alone: without them the same layout is taken
                    out = fp.twice(cs.entry, cs.body(("bits", "counts")), seed=400 + k, what=cs.tag() + " NULL byte masks")
                    cs.compare(out, [cs.reference(orc, f) for f in range(cs.N)], ("bits", "counts"), cs.tag() + " NULL byte masks")
                    cs.count()
                    ran += 1
        finally:
            cs.close()
    assert ran >= 3 and ran_z >= 1 and ran_padded >= 1, (f"the fused compaction without byte masks ran on {ran} layouts, {ran_z} with depth "
                                                          f"planes, {ran_padded} with a padded pitch")
    for entry in ("mdvt_render_stereo", "mdvt_render_stereo_batch"):
        print("\n" + fp.table([entry]))


@pytest.mark.parametrize("W,H", [(1, 1), (1, 5), (7, 1)])
def test_render_and_edge_filter_refuse_frames_below_2x2(mods, W, H):
    _lib, sr, synthetic = mods
    rng = np.random.default_rng(W + 10 * H)
    cs = RenderCase(mods, "points_fast", rng, fp.Layouts(rng), W, H, 1, sbs=False)
    try:
        fp.refused("mdvt_render_stereo", cs.body(("mask", "depth", "bits", "counts"), status=INVALID), INVALID)

        def body(run):
            d = run.inp("depth_rgb", cs.depth.reshape(1, H, 3 * W), fp.Layout(1, 3, 0))
            tri = run.out("tri_invalid", 1, 64, 1, fp.Layout(1, 0, 0))
            unused = run.out("unused", 1, H * W, 1, fp.Layout(3, 0, 0))
            K = (C.c_double * 9)(*[cs.ps[0].K[k] for k in range(9)])
            return _lib.load().mdvt_edge_filter(cs.r.ctx.handle, _vp(d), d.pitch, K, 1.0, 1, _vp(tri), _vp(unused), None)
        fp.refused("mdvt_edge_filter", body, INVALID)
    finally:
        cs.close()


FULL = [("points_fast", 1920, 1080, 0), ("points_general", 3840, 2160, 2), ("points_edges1", 1920, 1080, 0), ("mesh_band", 1920, 1080, 0),
        ("mesh_conv", 1920, 1080, 1), ("mesh_general", 3840, 2160, 2), ("mesh_edges1", 1920, 1080, 1), ("mesh_edges1", 1920, 1080, 0)]


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("family,W,H,kind", FULL)
def test_render_full_size(mods, orc, monkeypatch, family, W, H, kind, aligned):
    """One full-size frame per kernel family (3840 x 2160 for the posed 4K paths of the bench), separate eye buffers, padded
    pitches: once at an odd base offset (the byte paths) and once on a layout the vector kernels take (bases and paddings in
    multiples of 4, depth planes of 16: k_mesh_band, k_mesh_conv, the vec4 point rows at full size).  Properties 1, 2 and 4 in full; property 3 against the oracle for points, and for the mesh against the
    same frame rendered by a fresh context into tight side-by-side tensors (what the full-size tests hold to the oracle)."""
    _lib, sr, synthetic = mods
    if family == "mesh_conv":
        monkeypatch.setenv("MDVT_LIB_VARIANT", "tuning")
        monkeypatch.setenv("MDVT_MESH_CONV", "1")
    rng = np.random.default_rng(W + H + kind)
    lays = fp.Layouts(rng, (3, 20, 0)) if family != "mesh_band" else fp.Layouts(rng, (1, 3, 0))
    if aligned:
        lays = fp.Layouts(rng, (4, 20, 4), vec=True)
    cs = RenderCase(mods, family, rng, lays, W, H, 1, sbs=False, kinds=[kind], conv=8.0)
    cs.depth[0], cs.color[0] = synthetic.SyntheticScene(W, H, config_id=2).frame(3)
    full = ("mask",) + cs.optional
    try:
        out = fp.twice(cs.entry, cs.body(full), seed=W + kind, what=cs.tag())
        if family.startswith("points"):
            want = cs.reference(orc, 0)
        else:
            r2 = sr.StereoRerenderer(W, H, pupillary_distance=cs.ipd, **cs.kw)
            got = r2.render(torch.from_numpy(cs.depth[0]).cuda(), torch.from_numpy(cs.color[0]).cuda(), cs.ps[0], want_depth=True,
                            want_seed=r2.remove_edges)
            want = {}
            for e, eye in enumerate(("left", "right")):
                sl = slice(e * W, (e + 1) * W)
                want[eye + "_rgb"], want[eye + "_mask"] = got["sbs"][:, sl].cpu().numpy(), got["mask"][:, sl].cpu().numpy()
                want[eye + "_depth"] = got["depth"][:, sl].cpu().numpy()
                if r2.remove_edges:
                    want[eye + "_seed"] = got["seed"][:, sl].cpu().numpy()
            r2.close()
        cs.compare(out, [want], full, cs.tag())
        assert cs.count() == aligned, cs.tag() + ": the full-size case did not take the path it was laid out for"
    finally:
        cs.close()
    fp.finish_entry("mdvt_render_stereo", need_vector=aligned)


def _two_bank_sets(cs):
    """Frames per launch set of a run of general frames (chunk_of in mdvt_api.hip; include/mdvt.h, workspace_mib): 4 for points; for
    the mesh what the budget affords at 64 B per pixel and slot (+ 28 with edge points, + 3 with edge removal), at most 16."""
    if cs.r.mode == 0:
        return 4
    per_slot = cs.W * cs.H * (64 + (28 if cs.r.edge_points else 0) + (3 if cs.r.remove_edges else 0))
    return min(16, ((cs.kw.get("workspace_mib") or 4096) << 20) // per_slot)


@pytest.mark.parametrize("family", ["points_general", "points_edges1", "mesh_general", "mesh_edges1", "mesh_edges0"])
def test_render_long_batches_on_two_banks(mods, orc, family):
    """A run of posed (or converged) frames longer than one launch set, WITHOUT packed mask and hole counts: the sets take turns on
    two halves of the workspace and every second one runs on the library's own stream (mdvt_render_stereo_batch) -- which then
    writes into the caller's buffers.  The precondition is asserted: one run, more frames than a set holds, sets of at least 2."""
    edges = family != "points_general" and family != "mesh_general"
    ran = 0
    for k, (rng, lays) in enumerate(fp.layout_sweep(1, 601)):
        if k not in (0, 2, fp.FIRST_ODD, fp.FIRST_VEC, fp.FIRST_VEC + 2):
            continue
        _size.vec = lays.vec
        W = int(rng.choice((128, 252, 256) if lays.vec else (127, 129, 250, 257)))
        H = int(rng.choice((13, 19)))
        _size.vec = False
        per_slot = W * H * (64 + 28 + 3)
        ws_mib = max(1, -(-4 * per_slot // (1 << 20)))
        kind = (2, 1, 3)[k % 3]
        probe = RenderCase(mods, family, rng, fp.Layouts(rng, (0, 0, 0)), W, H, 1, sbs=False, ws_mib=ws_mib, kinds=[kind])
        chunk = _two_bank_sets(probe)
        probe.close()
        N = chunk + 3
        cs = RenderCase(mods, family, rng, lays, W, H, N, sbs=bool(k % 2) and not lays.vec, ws_mib=ws_mib, kinds=[kind] * N)
        want = ("mask", "depth") + (("seed",) if edges else ())
        tag = cs.tag() + f" sets of {chunk}"
        assert chunk >= 2 and N > chunk and "bits" not in want and "counts" not in want, tag
        try:
            out = fp.twice(cs.entry, cs.body(want), seed=600 + k, what=tag)
            cs.compare(out, [cs.reference(orc, f) for f in range(N)], want, tag)
            cs.count()
            ran += 1
        finally:
            cs.close()
    assert ran >= 4
    fp.finish_entry("mdvt_render_stereo_batch", need_vector=True)


# ------------------------------------------------------------------------------------------------- the stand-alone entry points
def _ctx(mods, W, H, **kw):
    _lib, sr, _ = mods
    return sr.StereoRerenderer(W, H, pupillary_distance=65, **kw)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sweep(entry, n_random, seed, case, need_vector=True):
    """case(rng, lays, k) runs one accepted layout (and whatever refusals it wants)."""
    for k, (rng, lays) in enumerate(fp.layout_sweep(n_random, seed)):
        _size.vec = "wide" if lays.vec and k == fp.FIRST_VEC + len(fp.VEC_FIXED) - 1 else lays.vec
        try:
            W = case(rng, lays, k)
        finally:
            _size.vec = False
        # the dword / vector paths of the stand-alone kernels take W % 4 == 0 with every pointer, pitch and stride a multiple of 4
        vector = W % 4 == 0 and fp.all_aligned(fp.LAST_RUN, 4)
        assert vector or not lays.vec, f"{entry}: a layout made for the vector path is not dword aligned (W = {W})"
        fp.accepted(entry, vector=vector)
    # (need_vector=False: the entry point's outputs are tight arrays without a pitch -- nothing to pad)
    fp.finish_entry(entry, need_vector=need_vector)


def test_decode_depth(mods, orc):
    entry = "mdvt_decode_depth"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, wide=True)
        rgb = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        md, sc = ((100.0, 1.0), (20.0, 1.3938468501173518))[k % 2]
        li, lo = lays.u8(), lays.w32()
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("rgb", rgb.reshape(1, H, 3 * W), li)
            o = run.out("depth", H, 4 * W, 1, lo)
            rc = L.mdvt_decode_depth(r.ctx.handle, _vp(a), a.pitch, _vp(o), 4 * W - 4 if short else o.pitch, md, sc, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} {li} {lo}")
        assert np.array_equal(out["depth"].view(np.uint32).reshape(H, W), orc.decode_depth(rgb[0], md, sc).view(np.uint32)), (W, H, li, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 14, 501, case)


def test_encode_depth(mods, orc):
    entry = "mdvt_encode_depth"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, wide=True)
        depth = rng.uniform(-5, 120, (1, H, W)).astype(np.float32)
        depth[0, 0, 0] = np.nan
        li, lo = lays.w32(), lays.u8()
        bgr = k % 2
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("depth", depth, li)
            o = run.out("rgb", H, 3 * W, 1, lo)
            rc = L.mdvt_encode_depth(r.ctx.handle, _vp(a), a.pitch, _vp(o), 3 * W - 1 if short else o.pitch, 100.0, bgr, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} {li} {lo}")
        want = orc.encode_depth(depth[0], 100)
        assert np.array_equal(out["rgb"].reshape(H, W, 3), want[..., ::-1] if bgr else want), (W, H, li, lo, bgr)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 14, 502, case)


def test_edge_filter(mods, orc):
    """Both outputs, and each alone (either may be NULL); they are tight arrays, so their arenas have base offsets only."""
    entry = "mdvt_edge_filter"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, 2, 2, wide=True)
        d = _depth_scene(rng, W, H)
        li = lays.u8()
        bt, bu = (int(rng.choice(fp.BASES4 if lays.vec else fp.BASES)) for _ in range(2))
        obo = k % 2
        r = _ctx(mods, W, H, remove_edges=True, render_as_pointcloud=not obo)
        p = r.frame_params(xfov=45.0)
        K = (C.c_double * 9)(*[p.K[q] for q in range(9)])
        nt = 2 * (H - 1) * (W - 1)

        def body(which, short=False):
            def run_body(run):
                a = run.inp("depth_rgb", d.reshape(1, H, 3 * W), li)
                t = run.out("tri_invalid", 1, nt, 1, fp.Layout(bt, 0, 0)) if "t" in which else None
                u = run.out("unused", 1, H * W, 1, fp.Layout(bu, 0, 0)) if "u" in which else None
                rc = L.mdvt_edge_filter(r.ctx.handle, _vp(a), 3 * W - 1 if short else a.pitch, K, p.depth_scale, obo,
                                        _vp(t) if t else None, _vp(u) if u else None, _stream())
                if not short:
                    r.ctx.check(rc)
                return rc
            return run_body
        wt, wu, _ = orc.edge_filter(orc.decode_depth(d, 100, p.depth_scale), _K(p), bool(obo))
        for which in (("tu",) if k % 3 else ("tu", "t", "u")):
            out = fp.twice(entry, body(which), seed=k, what=f"{W}x{H} {li} outputs={which}")
            if "t" in which:
                assert np.array_equal(out["tri_invalid"].reshape(-1), wt), (W, H, li, which)
            if "u" in which:
                assert np.array_equal(out["unused"].reshape(-1), wu), (W, H, li, which)
        if k % 4 == 0:
            fp.refused(entry, body("tu", True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 12, 503, case, need_vector=False)


def test_edge_point_pixels(mods, orc):
    entry = "mdvt_edge_point_pixels"
    _lib, sr, synthetic = mods
    from oracle import oracle_np as onp
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, 2, 2)
        d = _depth_scene(rng, W, H)
        li = lays.u8()
        lo = fp.Layout(int(rng.choice(fp.BASES4)), 0, 0)
        mesh = bool(k % 2)
        kind = (0, 0, 1, 2)[k % 4]
        T = synthetic.synthetic_pose_track(64)[7] if kind == 2 else None
        r = _ctx(mods, W, H, infill_mask=True, render_as_pointcloud=not mesh)
        p = r.frame_params(xfov=60.0, convergence_distance=2.5 if kind == 1 else None, transformation=T)
        depth = orc.decode_depth(d, 100.0, p.depth_scale)
        want, _, _ = onp.edge_point_chain(depth, _K(p), _K(p), W, H, mesh, 0.065, p.convergence_angle, T)
        inside = (want[..., 0] >= 0) & (want[..., 0] < W) & (want[..., 1] >= 0) & (want[..., 1] < H) & (depth.reshape(-1) > 1e-4)[:, None]
        for how in ((0, 1) if kind == 0 else (0,)):
            def body(run, short=False):
                a = run.inp("depth_rgb", d.reshape(1, H, 3 * W), li)
                o = run.out("px", H, 16 * W, 1, lo)
                rc = L.mdvt_edge_point_pixels(r.ctx.handle, C.byref(p), _vp(a), 3 * W - 1 if short else a.pitch, how, _vp(o), _stream())
                if not short:
                    r.ctx.check(rc)
                return rc
            out = fp.twice(entry, body, seed=k, what=f"{W}x{H} how={how} {li} {lo}")
            got = out["px"].view(np.int32).reshape(H * W, 2, 2).astype(np.int64)
            assert np.array_equal(got[inside], want[inside]) and np.all(got[~inside] == IMIN), (W, H, how, kind, mesh)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 8, 504, case, need_vector=False)


def _march_scene(rng, W, H):
    color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    hole = rng.uniform(size=(H, W)) < 0.05
    for _ in range(3):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        hole[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, max(2, W // 3)))] = True
    normal = rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)
    return color, hole.astype(np.uint8), normal


def test_infill_using_normals(mods, orc):
    entry = "mdvt_infill_using_normals"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng)
        color, hole, normal = _march_scene(rng, W, H)
        lc, lh, ln, lo = lays.u8(), lays.u8(), lays.w32(), lays.u8()
        r = _ctx(mods, W, H)

        def body(run, short=False):
            c = run.inp("color", color.reshape(1, H, 3 * W), lc)
            h = run.inp("hole", hole[None], lh)
            n = run.inp("normal", normal.reshape(1, H, 3 * W), ln)
            o = run.out("out", H, 3 * W, 1, lo)
            rc = L.mdvt_infill_using_normals(r.ctx.handle, _vp(c), c.pitch, _vp(h), h.pitch, _vp(n), n.pitch, _vp(o),
                                             3 * W - 1 if short else o.pitch, 400, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} {lc} {lh} {ln} {lo}")
        assert np.array_equal(out["out"].reshape(H, W, 3), orc.infill_using_normals(color, hole.astype(bool), normal)), (W, H, lc, lh, ln, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 12, 505, case)


def _ni_scene(rng, W, H):
    from test_gpu_normal_infill import ni_scene
    return ni_scene(rng, W, H, holes=5)


def test_mark_lower_side(mods, orc):
    entry = "mdvt_mark_lower_side"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng)
        _, img = _ni_scene(rng, W, H)
        li, lo = lays.u8(), lays.u8()
        steps = (30, 5)[k % 2]
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("img", img.reshape(1, H, 3 * W), li)
            o = run.out("out", H, 3 * W, 1, lo)
            rc = L.mdvt_mark_lower_side(r.ctx.handle, _vp(a), a.pitch, _vp(o), 3 * W - 1 if short else o.pitch, steps, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} {li} {lo}")
        assert np.array_equal(out["out"].reshape(H, W, 3), orc.mark_lower_side(img, steps)), (W, H, li, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 12, 506, case)


def test_touchly_depth(mods):
    """sr:549-551 evaluated literally with NumPy, as test_touchly_depth_plane does."""
    entry = "mdvt_touchly_depth"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, wide=True)
        depth = rng.uniform(0, 8, (1, H, W)).astype(np.float32)
        depth[0, rng.integers(H), rng.integers(W)] = 0
        tmax, tmin = ((5, 0), (5.0, 0.5), (12.5, 1.0))[k % 3]
        zif = k % 2
        li, lo = lays.w32(), lays.u8()
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("depth", depth, li)
            o = run.out("rgb", H, 3 * W, 1, lo)
            rc = L.mdvt_touchly_depth(r.ctx.handle, _vp(a), a.pitch, _vp(o), 3 * W - 1 if short else o.pitch, float(tmax), float(tmin), zif,
                                      _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} {li} {lo}")
        d8 = np.rint(np.maximum(0, np.minimum(depth[0], tmax) - tmin) * (255 / (tmax - tmin))).astype(np.uint8)
        if zif:
            d8[d8 == 0] = 255
        want = np.repeat((255 - d8)[..., np.newaxis], 3, axis=-1)
        assert np.array_equal(out["rgb"].reshape(H, W, 3), want), (W, H, li, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 14, 507, case)


def test_equirect_tables(mods, orc):
    """Host arrays (no context, no device work): arenas in host memory."""
    entry = "mdvt_equirect_tables"
    _lib, sr, _ = mods
    L = _lib.load()
    f32p = C.POINTER(C.c_float)

    def case(rng, lays, k):
        W, H = _size(rng, 2, 2, wide=True)
        fov = float(rng.choice([75.0, 100.0, 120.5]))
        bx, by = int(rng.choice(fp.BASES4)), int(rng.choice(fp.BASES4))

        def body(run, bad=False):
            x = run.out("map_x", 1, 4 * W, 1, fp.Layout(bx, 0, 0), device="cpu")
            y = run.out("map_y", 1, 4 * H, 1, fp.Layout(by, 0, 0), device="cpu")
            rc = L.mdvt_equirect_tables(W, H, 180.0 if bad else fov, C.cast(x.ptr, f32p), C.cast(y.ptr, f32p))
            assert bad or rc == 0
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H}", device="cpu")
        mx, my = orc.equirect_tables(W, H, fov)
        assert np.array_equal(out["map_x"].view(np.uint32).reshape(-1), mx.view(np.uint32))
        assert np.array_equal(out["map_y"].view(np.uint32).reshape(-1), my.view(np.uint32))
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k, device="cpu")
    for k, (rng, lays) in enumerate(fp.layout_sweep(6, 508)):
        case(rng, lays, k)
        fp.tally(entry)["accepted"] += 1
    fp.finish_entry(entry, need_odd=False, need_padded=False)      # float arrays without a pitch: offsets in multiples of 4 only


def test_equirect_remap(mods, orc):
    entry = "mdvt_equirect_remap"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, 2, 2)
        N = 1 + k % 3
        fov = float(rng.choice([75.0, 100.0, 120.5]))
        img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        img[0, :, : W // 2] = np.linspace(0, 255, W // 2, dtype=np.uint8)[None, :, None]
        mx, my = orc.equirect_tables(W, H, fov)
        li, lo, lx, ly = lays.u8(), lays.u8(), fp.Layout(int(rng.choice(fp.BASES4))), fp.Layout(int(rng.choice(fp.BASES4)))
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("src", img.reshape(N, H, 3 * W), li)
            x = run.inp("map_x", mx.reshape(1, 1, W), lx)
            y = run.inp("map_y", my.reshape(1, 1, H), ly)
            o = run.out("dst", H, 3 * W, N, lo)
            rc = L.mdvt_equirect_remap(r.ctx.handle, _vp(a), a.pitch, a.stride, _vp(o), 3 * W - 1 if short else o.pitch, o.stride, N, _vp(x), _vp(y),
                                       _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} x{N} {li} {lo}")
        for f in range(N):
            assert np.array_equal(out["dst"][f].reshape(H, W, 3), orc.convert_to_equirectangular(img[f], fov)), (W, H, f, li, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 12, 509, case)


def test_swap_rb(mods):
    """Out of place and, every other case, in place (d_dst == d_src with equal pitch / stride, as the header allows)."""
    entry = "mdvt_swap_rb"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, wide=True)
        N = 1 + k % 3
        img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        li, lo = lays.u8(), lays.u8()
        in_place = k % 2 == 1
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("src", img.reshape(N, H, 3 * W), li, inout=in_place)
            o = a if in_place else run.out("dst", H, 3 * W, N, lo)
            rc = L.mdvt_swap_rb(r.ctx.handle, _vp(a), a.pitch, a.stride, _vp(o), 3 * W - 1 if short else o.pitch, o.stride, N, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} x{N} {li} {lo} in_place={in_place}")
        got = out["src" if in_place else "dst"]
        assert np.array_equal(got.reshape(N, H, W, 3), img[..., ::-1]), (W, H, N, li, lo, in_place)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 16, 510, case)


def test_masked_blur(mods, orc):
    entry = "mdvt_masked_blur"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[rng.uniform(size=(H, W)) < 0.4] = 0
        li, lo = lays.u8(), lays.u8()
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("img", img.reshape(1, H, 3 * W), li)
            o = run.out("out", H, 3 * W, 1, lo)
            rc = L.mdvt_masked_blur(r.ctx.handle, _vp(a), a.pitch, _vp(o), 3 * W - 1 if short else o.pitch, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} {li} {lo}")
        assert np.array_equal(out["out"].reshape(H, W, 3), orc.masked_blur(img)), (W, H, li, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 12, 511, case)


def _seed_image(rng, W, H, key=GREEN):
    """A seed image as the render hands it over: black, key-coloured holes, normal-coloured points on their rims."""
    seed = np.zeros((H, W, 3), np.uint8)
    for _ in range(3):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        w, h = int(rng.integers(1, max(2, W // 3))), int(rng.integers(1, max(2, H // 2)))
        seed[y0:y0 + h, x0:x0 + w] = key
        for _ in range(w + h):
            seed[min(H - 1, y0 + int(rng.integers(0, h))), min(W - 1, x0 + int(rng.integers(0, 2)))] = rng.integers(1, 255, 3)
    return seed


def _fmm_finish(orc, seed):
    from test_gpu_inpaint_heap import fmm_finish, unreachable_keys
    return fmm_finish(orc, seed), unreachable_keys(seed)


def _finish_cases(mods, orc, entry, stereo, heap):
    """The four completions share their shape: seeds in, finished masks out, d_remaining (handed over poisoned: "receives")."""
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng, max_w=129)
        N = 1 + k % 3
        eyes = 2 if stereo else 1
        seeds = np.stack([[_seed_image(rng, W, H) for _ in range(N)] for _ in range(eyes)])         # [eye, frame, H, W, 3]
        li, lo, lrem = lays.u8(), lays.u8(), fp.Layout(int(rng.choice(fp.BASES4)))
        rounds = 0 if heap else (0, 2, -40)[k % 3]                # all levels; a bound that leaves pixels; the asynchronous form
        bound = 65000 if rounds == 0 else abs(rounds)
        sbs = stereo and k % 2 == 0
        r = _ctx(mods, W, H, infill_mask=True)

        def body(with_rem, short=False):
            def run_body(run):
                if sbs:                                           # both eyes as column halves of one buffer
                    a = run.inp("seed", np.concatenate([seeds[0], seeds[1]], axis=2).reshape(N, H, 6 * W), li)
                    o = run.out("out", H, 6 * W, N, lo)
                    ptrs = (a.ptr, a.ptr + 3 * W, o.ptr, o.ptr + 3 * W)
                else:
                    a = run.inp("seed", seeds[0].reshape(N, H, 3 * W), li)
                    o = run.out("out", H, 3 * W, N, lo)
                    ptrs = (a.ptr, None, o.ptr, None)
                    if stereo:
                        a2 = run.inp("seed_right", seeds[1].reshape(N, H, 3 * W), fp.Layout((li.base + (4 if lays.vec else 1)) % 16, li.pad, li.gap))
                        o2 = run.out("out_right", H, 3 * W, N, fp.Layout((lo.base + (8 if lays.vec else 3)) % 16, lo.pad, lo.gap))
                        ptrs = (a.ptr, a2.ptr, o.ptr, o2.ptr)
                rem = run.out("remaining", 1, 4 * N * eyes, 1, lrem) if with_rem else None
                remp = _vp(rem) if rem else None
                op = 3 * W - 1 if short else o.pitch
                h = r.ctx.handle
                if stereo and heap:
                    rc = L.mdvt_finish_infill_mask_heap_stereo(h, ptrs[0], ptrs[1], a.pitch, a.stride, ptrs[2], ptrs[3], op, o.stride, N, remp, _stream())
                elif stereo:
                    rc = L.mdvt_finish_infill_mask_stereo(h, ptrs[0], ptrs[1], a.pitch, a.stride, ptrs[2], ptrs[3], op, o.stride, N, rounds, remp, _stream())
                elif heap:
                    rc = L.mdvt_finish_infill_mask_heap(h, ptrs[0], a.pitch, a.stride, ptrs[2], op, o.stride, N, remp, _stream())
                else:
                    rc = L.mdvt_finish_infill_mask(h, ptrs[0], a.pitch, a.stride, ptrs[2], op, o.stride, N, rounds, remp, _stream())
                if not short:
                    r.ctx.check(rc)
                return rc
            return run_body
        tag = f"{W}x{H} x{N} {li} {lo} rounds={rounds} sbs={sbs}"
        out = fp.twice(entry, body(True), seed=k, what=tag)
        rem = np.ascontiguousarray(out["remaining"]).view(np.uint32).reshape(eyes, N)           # left eyes first, then right eyes
        for e in range(eyes):
            for f in range(N):
                want, wrem = _fmm_finish(orc, seeds[e, f]) if heap else orc.finish_infill_mask(seeds[e, f], max_rounds=bound)
                got = out["out"][f][:, e * 3 * W:(e + 1) * 3 * W] if (sbs or e == 0) else out["out_right"][f]
                assert np.array_equal(got.reshape(H, W, 3), want), (tag, e, f)
                assert int(rem[e, f]) == wrem, (tag, e, f, int(rem[e, f]), wrem)
        none = fp.twice(entry, body(False), seed=k, what=tag + " without d_remaining")           # the optional output left out
        for name in none:
            assert np.array_equal(none[name], out[name]), (tag, name)
        if k % 4 == 0:
            fp.refused(entry, body(True, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 6, 520 + 2 * stereo + heap, case)


def test_finish_infill_mask(mods, orc):
    _finish_cases(mods, orc, "mdvt_finish_infill_mask", False, False)


def test_finish_infill_mask_stereo(mods, orc):
    _finish_cases(mods, orc, "mdvt_finish_infill_mask_stereo", True, False)


def test_finish_infill_mask_heap(mods, orc):
    _finish_cases(mods, orc, "mdvt_finish_infill_mask_heap", False, True)


def test_finish_infill_mask_heap_stereo(mods, orc):
    _finish_cases(mods, orc, "mdvt_finish_infill_mask_heap_stereo", True, True)


def test_normal_infill(mods, orc):
    entry = "mdvt_normal_infill"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng)
        N = 1 + k % 3
        pairs = [_ni_scene(rng, W, H) for _ in range(N)]
        img, mask = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        li, lm, lo = lays.u8(), lays.u8(), lays.u8()
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("img", img.reshape(N, H, 3 * W), li)
            m = run.inp("mask", mask.reshape(N, H, 3 * W), lm)
            o = run.out("out", H, 3 * W, N, lo)
            rc = L.mdvt_normal_infill(r.ctx.handle, _vp(a), a.pitch, a.stride, _vp(m), m.pitch, m.stride, _vp(o), 3 * W - 1 if short else o.pitch,
                                      o.stride, N, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} x{N} {li} {lm} {lo}")
        for f in range(N):
            assert np.array_equal(out["out"][f].reshape(H, W, 3), orc.normal_infill(img[f], mask[f])), (W, H, f, li, lm, lo)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 10, 530, case)


def test_infill_using_mask_normals(mods, orc):
    """d_img is in-out: its payload is an input, the call may change the hole pixels the march fills -- to what the oracle's
    infill_using_normals gives with the mask image's normals -- and nothing else; padding and guards as everywhere."""
    entry = "mdvt_infill_using_mask_normals"
    _lib, sr, _ = mods
    L = _lib.load()

    def case(rng, lays, k):
        W, H = _size(rng)
        N = 1 + k % 3
        img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        hole = np.stack([_march_scene(rng, W, H)[1] for _ in range(N)])
        mimg = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        li, lh, lm = lays.u8(), lays.u8(), lays.u8()
        r = _ctx(mods, W, H)

        def body(run, short=False):
            a = run.inp("img", img.reshape(N, H, 3 * W), li, inout=True)
            h = run.inp("hole", hole, lh)
            m = run.inp("mask_img", mimg.reshape(N, H, 3 * W), lm)
            rc = L.mdvt_infill_using_mask_normals(r.ctx.handle, _vp(a), a.pitch, a.stride, _vp(h), W - 1 if short else h.pitch, h.stride, _vp(m),
                                                  m.pitch, m.stride, N, 400, _stream())
            if not short:
                r.ctx.check(rc)
            return rc
        out = fp.twice(entry, body, seed=k, what=f"{W}x{H} x{N} {li} {lh} {lm}")
        for f in range(N):
            normals = ((mimg[f].astype(np.float32) / np.float32(255.0)) * 2 - 1).astype(np.float32)          # sr:808 + 810
            want = orc.infill_using_normals(img[f], hole[f].astype(bool), normals)
            got = out["img"][f].reshape(H, W, 3)
            assert np.array_equal(got, want), (W, H, f, li, lh, lm)
            assert np.array_equal(got[hole[f] == 0], img[f][hole[f] == 0]), "a pixel that is no hole changed"
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        r.close()
        return W
    _sweep(entry, 10, 531, case)


def test_encode_video_frames(mods):
    """The packet buffer of the stated capacity inside an arena: packets byte for byte the host encoder's, a size written
    for every frame (and an offset for every frame that got a packet), nothing beyond the capacity -- also where slices or the buffer overflow
    (test_overflow_falls_back_to_the_host_bytes' two constructions).  Bytes of the capacity behind the last packet are the
    call's (include/mdvt.h); the test holds the packets, the offsets and the sizes to property 2."""
    entry = "mdvt_encode_video_frames"
    _lib, sr, _ = mods
    from metric_depth_video_toolbox_amd import ffv1_device as fd, video_io
    L = _lib.load()
    ctx = _lib.Context(0, 16, 16)

    def case(rng, lays, k):
        W, H = _size(rng, 2, 2, max_w=129)
        N = 1 + k % 3
        ch = (3, 3, 1)[k % 3]
        bgr = k % 2
        slices = (min(2, W), min(2, H)) if k % 2 else (1, 1)
        frames = rng.integers(0, 256, (N, H, W, ch), dtype=np.uint8)
        frames[0, :, : W // 2] = 40                                        # a flat half: short packets
        if N > 1:
            frames[1] = 7                                                  # a flat frame: fits where noise does not
        host = [video_io.encode_frame(np.repeat(f, 3, axis=-1) if ch == 1 else f, slices=slices, bgr=bool(bgr), threads=1)[0] for f in frames]
        mode = k % 4                                     # 0, 1: room for all; 2: a slice capacity of 60 bytes; 3: a buffer for the first packet only
        slice_cap = 60 if mode == 2 else 0
        cap = len(host[0]) if mode == 3 else N * fd.packet_capacity_bytes(W, H, slices, slice_cap)
        li, lp = lays.u8(), lays.u8()
        loff, lsz = fp.Layout(int(rng.choice((0, 8)))), fp.Layout(int(rng.choice(fp.BASES4)))

        def body(run, short=False):
            a = run.inp("src", frames.reshape(N, H, W * ch), li)
            p = run.out("packets", 1, cap, 1, fp.Layout(lp.base, 0, 0))
            o = run.out("offsets", 1, 8 * N, 1, loff)
            s = run.out("sizes", 1, 4 * N, 1, lsz)
            rc = L.mdvt_encode_video_frames(ctx.handle, W, H, slices[0], slices[1], _vp(a), W * ch - 1 if short else a.pitch, a.stride, ch, bgr, N,
                                           slice_cap, _vp(p), cap, _vp(o), _vp(s), _stream())
            if not short:
                ctx.check(rc)
            return rc
        tag = f"{W}x{H} x{N} ch={ch} slices={slices} mode={mode} {li} {lp}"
        res = []
        for comp in (False, True):
            run = fp.Run(entry, comp, k)
            body(run)
            out = run.check()
            sizes = np.ascontiguousarray(out["sizes"]).view(np.uint32).reshape(-1)
            offs = np.ascontiguousarray(out["offsets"]).view(np.uint64).reshape(-1)
            pk = []
            for f in range(N):
                if sizes[f] < fd.TOO_LARGE:
                    assert int(offs[f]) + int(sizes[f]) <= cap, tag
                    pk.append(out["packets"].reshape(-1)[int(offs[f]):int(offs[f]) + int(sizes[f])].tobytes())
                else:
                    pk.append(None)
            res.append((sizes.copy(), pk))
        assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1], tag + ": sizes or packets differ between the two poisons"
        sizes, pk = res[0]
        for f in range(N):
            if sizes[f] < fd.TOO_LARGE:
                assert pk[f] == host[f], (tag, f)
            else:
                assert sizes[f] == fd.OVERFLOW and mode >= 2, (tag, f, hex(int(sizes[f])))
        if mode < 2:
            assert all(s < fd.TOO_LARGE for s in sizes), tag
        if mode == 3:
            assert sizes[0] == len(host[0]) and all(s == fd.OVERFLOW for s in sizes[1:]), (tag, sizes)
        if k % 4 == 0:
            fp.refused(entry, lambda run: body(run, True), INVALID, seed=k)
        fp.LAST_RUN = list(run.arenas.values())
        return W
    try:
        _sweep(entry, 10, 540, case, need_vector=False)
    finally:
        ctx.close()


def test_ffv1_encode_frame_on_the_host():
    """mdvt_ffv1_encode_frame (include/mdvt_video.h; the reference of the device encoder above): its packet and configuration
    buffers of a stated capacity in host arenas -- the same cases tests/test_footprint_cpu.py runs without a GPU, here for the table."""
    fp.ffv1_encode_frame_cases()


def test_the_table_names_every_entry_point(request):
    """Printed last: the whole table.  When the whole file ran (no -k, no node ids), every entry point must be in it."""
    print("\n" + fp.table())
    everything = set(fp.ENTRY_POINTS) | set(fp.HOST_VIDEO_ENTRY_POINTS)
    assert set(fp.TALLY) <= everything
    mine = {name for name, obj in globals().items() if name.startswith("test_") and callable(obj)}
    selected = {item.originalname for item in request.session.items if item.fspath == request.node.fspath}
    if mine <= selected:
        assert set(fp.TALLY) == everything, f"no footprint case ran for {sorted(everything - set(fp.TALLY))}"
        for e in everything:
            assert fp.tally(e)["accepted"] >= 1, e
