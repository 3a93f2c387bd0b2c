"""Footprint testing of the C ABI (include/mdvt.h): every buffer a call is handed lives inside an *arena*, one uint8 tensor

    [ guard | frame 0: rows x pitch | gap up to stride | frame 1 ... | guard ]

whose every byte outside the payload (the first `row_bytes` bytes of each row) holds a seeded pseudo-random *poison*, or that
poison's bitwise complement.  A case runs once on each; then

  1. nothing outside    no byte outside an output's payload changed, and no byte of an input at all (Run.check);
  2. everything inside  every payload byte is equal in the two runs -- a byte that was not written differs in all 8 bits, and a
                        result that depends on a byte beyond an input's payload differs too (compare_runs);
  3. right              the payload equals the reference (the tests' own business).

A stray store of up to a row's length stays inside the arena's tensor: a defect shows as a changed byte, never as a fault.
tests/test_gpu_footprint.py holds every device-writing entry point to this; tests/test_footprint_cpu.py keeps the list below in
step with the header.  Plain module: no fixture, no pytest setting."""
from __future__ import annotations

import os
import re

import numpy as np

GUARD = 4096

# every entry point of include/mdvt.h that writes memory the caller owns: test_gpu_footprint.py has a case family for each
ENTRY_POINTS = (
    "mdvt_render_stereo", "mdvt_render_stereo_batch", "mdvt_decode_depth", "mdvt_encode_depth", "mdvt_edge_filter",
    "mdvt_edge_point_pixels", "mdvt_infill_using_normals", "mdvt_mark_lower_side", "mdvt_touchly_depth", "mdvt_equirect_tables",
    "mdvt_equirect_remap", "mdvt_swap_rb", "mdvt_masked_blur", "mdvt_finish_infill_mask", "mdvt_finish_infill_mask_stereo",
    "mdvt_finish_infill_mask_heap", "mdvt_finish_infill_mask_heap_stereo", "mdvt_normal_infill", "mdvt_infill_using_mask_normals",
    "mdvt_encode_video_frames")

# entry points with a non-const pointer argument that is NOT an image buffer of the caller's
EXEMPT = {
    "mdvt_selftest": "h_mismatches: one host uint64",
    "mdvt_debug_read": "h_dst / info: host outputs of the tuning library's diagnosis",
    "mdvt_workspace_bytes": "bytes: one host uint64",
    "mdvt_cached_memory": "idle_bytes / idle_blocks: host uint64s",
}

# widths around every store width and path switch (16-byte and 8-byte stores, dwords of the packed mask, W % 4)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 250, 255, 257)
# test_widths_around_the_lds_limits and test_mesh_wide_frames_use_compact_lds_vertices
LDS_WIDTHS = (10236, 10240, 6824, 6828, 4296, 4300, 5120, 3840, 4600, 5000)
HEIGHTS = (1, 2, 3, 5, 7, 11, 13, 19)          # 7 ... 19: no multiple of the band heights 2, 3, 5, 8 (test_mesh_band_heights)
BASES = (0, 1, 2, 3, 4, 8, 12)
PADS = (0, 1, 3, 4, 20)
BASES4 = (0, 4, 8, 12)                          # float and dword planes
PADS4 = (0, 4, 12, 16, 20, 32)                  # pitches that are and are not multiples of 16


def raw_io(_lib, **kw):
    io = _lib.MdvtIO()
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def header_entry_points(path):
    """{name: argument text} of every `int mdvt_*(` declaration of the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(mdvt_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def writes_through_a_pointer(args):
    """True if an argument list has a pointer to non-const data other than the context, the stream or a struct passed by const *."""
    for a in args.split(","):
        a = a.strip()
        if "*" not in a or a.startswith("const ") or a.startswith("mdvt_ctx*") or a.startswith("void* stream"):
            continue
        return True
    return False


class Layout:
    """Where a buffer sits: bytes past a 256-byte boundary, bytes of padding per row, bytes of gap per frame."""

    def __init__(self, base=0, pad=0, gap=0):
        self.base, self.pad, self.gap = int(base), int(pad), int(gap)

    def __repr__(self):
        return f"+{self.base}/pad{self.pad}/gap{self.gap}"


class Layouts:
    """One case's layouts, drawn from `rng`; `fixed` pins (base, pad) of every u8 buffer (the systematic part of a sweep)."""

    def __init__(self, rng, fixed=None, vec=False):
        # vec: a layout the vector paths accept ON PURPOSE (plan.vec4 of the render, the dword paths of the stand-alone kernels):
        # bases, paddings and gaps in multiples of 4, float / dword planes in multiples of 16 -- with padding and gaps; the case
        # then takes a width that is a multiple of 4, at least 8
        self.rng, self.fixed, self.drawn, self.vec = rng, fixed, [], bool(vec)

    def _keep(self, lay):
        self.drawn.append(lay)
        return lay

    def u8(self, gap_unit=1):
        if self.fixed is not None:
            return self._keep(Layout(self.fixed[0], self.fixed[1], self.fixed[2] * gap_unit))
        r = self.rng
        return self._keep(Layout(r.choice(BASES), r.choice(PADS), int(r.choice((0, 0, 5, 64))) * gap_unit))

    def w32(self):
        """float / dword planes: offsets and pitches in multiples of 4."""
        r = self.rng
        if self.vec:
            return self._keep(Layout(0, 16 if self.fixed[1] % 8 else 32, 16 if self.fixed[2] else 0))
        if self.fixed is not None:
            return self._keep(Layout(self.fixed[0] & ~3, (self.fixed[1] + 3) & ~3, 4 * self.fixed[2]))
        return self._keep(Layout(r.choice(BASES4), r.choice(PADS4), int(r.choice((0, 0, 16, 40)))))

    @property
    def odd_base(self):
        return any(l.base % 2 for l in self.drawn)

    @property
    def padded(self):
        return any(l.pad for l in self.drawn)


# (base, pad, gap) of the vector-eligible layouts: the smallest alignment the vector paths accept, padded pitches, gaps
VEC_FIXED = ((4, 4, 4), (8, 20, 0), (12, 12, 64), (0, 4, 0))
FIRST_VEC, FIRST_ODD = 10, 4                    # indices into layout_sweep: its first vector-eligible and its first odd-base layout


def layout_sweep(n_random, seed):
    """The layouts of one entry point's cases: first every base offset with a pitch padding that cycles through PADS (all of a
    case's buffers alike: tight and aligned first, so the vector paths are reached with each alignment), then n_random cases whose
    buffers each draw their own.  MDVT_SWEEP_SEED / MDVT_SWEEP_CASES widen it as they widen sweep_cases."""
    rng = np.random.default_rng(int(os.environ.get("MDVT_SWEEP_SEED", "20261016")) + seed)
    n_random = int(os.environ.get("MDVT_SWEEP_CASES", n_random))
    fixed = [(0, 0, 0), (4, 4, 0), (0, 20, 1), (8, 0, 4)] + [(b, PADS[k % len(PADS)], k % 2) for k, b in enumerate(BASES[1:])]
    for f in fixed:
        yield rng, Layouts(rng, f)
    for f in VEC_FIXED:
        yield rng, Layouts(rng, f, vec=True)
    for _ in range(n_random):
        yield rng, Layouts(rng)


class Arena:
    def __init__(self, rows, row_bytes, pitch=None, n_frames=1, stride=None, base_offset=0, guard=GUARD, *, seed=0,
                 complement=False, device="cuda", name=""):
        import torch
        self.rows, self.row_bytes, self.n_frames = int(rows), int(row_bytes), int(n_frames)
        self.pitch = int(row_bytes if pitch is None else pitch)
        self.stride = int(self.rows * self.pitch if stride is None else stride)
        assert self.rows >= 1 and self.row_bytes >= 1 and self.n_frames >= 1
        assert self.pitch >= self.row_bytes and self.stride >= self.rows * self.pitch and 0 <= base_offset < 16
        # (a stray store of a row's length, from any row, stays inside the tensor)
        self.guard = max(int(guard), GUARD, 2 * self.pitch)
        self.base_offset, self.name, self.complement = int(base_offset), name, bool(complement)
        self.span = (self.n_frames - 1) * self.stride + self.rows * self.pitch
        total = self.guard + 256 + self.span + self.guard
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        self.start = self.guard + (self.base_offset - (self.buf.data_ptr() + self.guard)) % 256
        # the poison is a function of (seed, position relative to the payload's start): the same bytes wherever the tensor lies
        p = np.random.default_rng([int(seed), 0x6d647674]).integers(0, 256, total + 256, dtype=np.uint8)
        self.poison = p[256 - (self.start - self.guard):][:total].copy()
        if self.complement:
            self.poison = ~self.poison
        self.inside = np.zeros(total, bool)
        self._view(self.inside)[...] = True
        self.input = None
        self.inout = False
        self.buf.copy_(torch.from_numpy(self.poison))

    def _view(self, host):
        return np.lib.stride_tricks.as_strided(host[self.start:], shape=(self.n_frames, self.rows, self.row_bytes),
                                               strides=(self.stride, self.pitch, 1))

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    @property
    def outside_bytes(self):
        return int(self.inside.size - self.inside.sum())

    def write(self, data, inout=False):
        """Payload := data (any dtype, n_frames x rows x row_bytes bytes), the rest stays poison."""
        import torch
        d = np.ascontiguousarray(data).view(np.uint8).reshape(self.n_frames, self.rows, self.row_bytes)
        host = self.poison.copy()
        self._view(host)[...] = d
        self.buf.copy_(torch.from_numpy(host))
        self.input, self.inout = d.copy(), bool(inout)
        return self

    def read(self):
        return self.buf.cpu().numpy()

    def payload(self, host=None, dtype=np.uint8):
        host = self.read() if host is None else host
        return np.ascontiguousarray(self._view(host)).view(dtype)

    def where(self, off):
        rel = int(off) - self.start
        if rel < 0:
            return f"guard before the payload, {-rel} bytes before its first byte"
        if rel >= self.span:
            return f"guard after the payload, {rel - self.span} bytes past the last row's end"
        f, r = divmod(rel, self.stride)
        if r >= self.rows * self.pitch:
            return f"gap after frame {f}, byte {r - self.rows * self.pitch}"
        row, b = divmod(r, self.pitch)
        return f"(frame {f}, row {row}, byte {b}) = pitch padding, {b - self.row_bytes} bytes past the row's end"

    def changed(self, host=None):
        """Offsets outside the payload that no longer hold their poison."""
        host = self.read() if host is None else host
        return np.flatnonzero((host != self.poison) & ~self.inside)

    def report(self, host, offs, limit=6):
        lines = [f"{self.name or 'arena'}: {len(offs)} byte(s) outside the payload changed "
                 f"(rows {self.rows} x {self.row_bytes} B, pitch {self.pitch}, {self.n_frames} frame(s), stride {self.stride}, base +{self.base_offset})"]
        for o in offs[:limit]:
            lines.append(f"  {self.where(o)}: poison 0x{int(self.poison[o]):02x}, found 0x{int(host[o]):02x}")
        return "\n".join(lines)


TALLY = {}


LAST_RUN = None                                  # the arenas of the last run that twice() accepted: what accepted() counts from


def tally(entry):
    return TALLY.setdefault(entry, dict(accepted=0, refused=0, odd_base=0, padded=0, vector_padded=0, outside_bytes=0))


def all_aligned(arenas, unit=4):
    """Every pointer, pitch and stride of the arenas a multiple of `unit`."""
    return all(a.ptr % unit == 0 and (a.rows == 1 or a.pitch % unit == 0) and (a.n_frames == 1 or a.stride % unit == 0) for a in arenas)


def table(entries=None):
    rows = ["entry point                           accepted  refused  odd base  padded pitch  vector path + padded  guard+padding bytes checked"]
    for e in (entries or sorted(TALLY)):
        t = tally(e)
        rows.append(f"{e:<37} {t['accepted']:>8} {t['refused']:>8} {t['odd_base']:>9} {t['padded']:>13} {t['vector_padded']:>21} {t['outside_bytes']:>28}")
    return "\n".join(rows)


def finish_entry(entry, need_odd=True, need_padded=True, need_vector=False):
    """Print the entry point's row and insist on its coverage (called at the end of its test)."""
    print("\n" + table([entry]))
    t = tally(entry)
    assert t["accepted"] >= 1, f"{entry}: no accepted layout ran"
    assert not need_odd or t["odd_base"] >= 1, f"{entry}: no accepted layout with an odd base offset"
    assert not need_padded or t["padded"] >= 1, f"{entry}: no accepted layout with a padded pitch"
    assert not need_vector or t["vector_padded"] >= 1, f"{entry}: no accepted layout that reaches the vector path with a padded pitch"


class Run:
    """The arenas of one run of one case, all on poison P (complement=False) or on ~P."""

    def __init__(self, entry, complement, seed=1, device="cuda"):
        self.entry, self.complement, self.seed, self.device = entry, bool(complement), int(seed), device
        self.arenas = {}

    def _arena(self, name, rows, row_bytes, n_frames, lay, device=None):
        lay = lay or Layout()
        pitch = row_bytes + lay.pad
        a = Arena(rows, row_bytes, pitch, n_frames, rows * pitch + lay.gap, lay.base, seed=self.seed * 1000 + len(self.arenas),
                  complement=self.complement, device=device or self.device, name=f"{self.entry} {name} {lay}")
        a.lay = lay
        self.arenas[name] = a
        return a

    def inp(self, name, data, lay=None, inout=False, device=None):
        """data: [n_frames, rows, ...] (the trailing axes are one row)."""
        d = np.ascontiguousarray(data)
        d = d.reshape(d.shape[0], d.shape[1], -1)
        row_bytes = d.shape[2] * d.dtype.itemsize
        return self._arena(name, d.shape[1], row_bytes, d.shape[0], lay, device).write(d, inout)

    def out(self, name, rows, row_bytes, n_frames=1, lay=None, device=None):
        return self._arena(name, rows, row_bytes, n_frames, lay, device)

    def check(self, untouched=False):
        """Property 1 for every arena of the run; inputs must come back byte for byte.  untouched: a refused call -- nothing at
        all may have changed.  -> {name: payload} of the outputs and in-out buffers."""
        import torch
        if self.device != "cpu":
            torch.cuda.synchronize()
        res, t = {}, tally(self.entry)
        for name, a in self.arenas.items():
            host = a.read()
            offs = a.changed(host)
            assert offs.size == 0, a.report(host, offs)
            t["outside_bytes"] += a.outside_bytes
            pay = a.payload(host)
            if a.input is not None and not a.inout:
                assert np.array_equal(pay, a.input), f"{a.name}: the call changed its input"
            elif untouched:
                want = a.input if a.input is not None else a.payload(a.poison)
                assert np.array_equal(pay, want), f"{a.name}: a refused call wrote into the buffer"
            else:
                res[name] = pay
        return res


def compare_runs(entry, a, b, what=""):
    """Property 2 (and 4): the payloads of the run on P and of the run on ~P are equal."""
    assert a.keys() == b.keys()
    for k in a:
        if np.array_equal(a[k], b[k]):
            continue
        bad = np.argwhere(a[k] != b[k])
        f, r, x = (int(v) for v in bad[0])
        flipped = int(((a[k] ^ b[k]) == 0xFF).sum())
        raise AssertionError(
            f"{entry} {what}: output '{k}' differs between the run on the poison and the run on its complement at {len(bad)} byte(s), "
            f"{flipped} of them in all 8 bits (= never written); first at (frame {f}, row {r}, byte {x}): "
            f"0x{int(a[k][f, r, x]):02x} vs 0x{int(b[k][f, r, x]):02x}.  A byte that is not written, accumulated into, or computed "
            f"from bytes outside an input's payload shows up here.")


def twice(entry, body, seed=1, what="", device="cuda"):
    """body(run) builds its arenas on `run`, makes the call(s) and returns nothing; -> the outputs' payloads, after properties 1, 2
    and 4 have been checked."""
    global LAST_RUN
    res = []
    for comp in (False, True):
        run = Run(entry, comp, seed, device)
        body(run)
        res.append(run.check())
    compare_runs(entry, res[0], res[1], what)
    LAST_RUN = list(run.arenas.values())
    return res[0]


def refused(entry, body, status, seed=1, device="cuda"):
    """A layout the ABI refuses: body(run) returns the status of the call; every arena must be as it was."""
    for comp in (False, True):
        run = Run(entry, comp, seed, device)
        rc = body(run)
        assert rc == status, f"{entry}: expected status {status} for a layout the header refuses, got {rc}"
        run.check(untouched=True)
    tally(entry)["refused"] += 1


def accepted(entry, vector=False, arenas=None):
    """Count the case twice() just accepted, from the arenas it really allocated.  vector: the case's own predicate says the call
    took its vector path (the render's plan.vec4, a stand-alone kernel's dword path).  -> (odd base, padded, vector and padded)"""
    arenas = LAST_RUN if arenas is None else arenas
    t = tally(entry)
    odd = any(a.base_offset % 2 for a in arenas)
    padded = any(a.rows > 1 and a.pitch > a.row_bytes for a in arenas)
    out_padded = any(a.rows > 1 and a.pitch > a.row_bytes and (a.input is None or a.inout) for a in arenas)
    t["accepted"] += 1
    t["odd_base"] += int(odd)
    t["padded"] += int(padded)
    t["vector_padded"] += int(bool(vector) and out_padded)
    return odd, padded, bool(vector) and out_padded


# entry points of include/mdvt_video.h with a caller-owned output buffer of a stated capacity (host memory)
HOST_VIDEO_ENTRY_POINTS = ("mdvt_ffv1_encode_frame",)


def ffv1_encode_frame_cases(n_random=6, seed=550):
    """mdvt_ffv1_encode_frame (host): packet and configuration record written into arenas of exactly their size, of a generous
    size and of one byte too few (MDVT_VIDEO's argument error, nothing touched); the source frame in a padded, offset arena.
    Needs no GPU; the reference is tests/../oracle/ffv1_ref.py's independent decoder: the packet must decode to the frame."""
    import ctypes as C
    from metric_depth_video_toolbox_amd import video_io
    from oracle import ffv1_ref
    entry = "mdvt_ffv1_encode_frame"
    L = video_io.load()
    for k, (rng, lays) in enumerate(layout_sweep(n_random, seed)):
        W, H = int(rng.choice((2, 3, 5, 8, 17, 33, 64))), int(rng.choice((2, 3, 5, 13)))
        slices = (min(2, W), min(2, H)) if k % 2 else (1, 1)
        frame = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        frame[0, :, : W // 2] = 40
        want_pkt, want_cfg = video_io.encode_frame(frame[0], slices=slices, bgr=bool(k % 2), threads=1)
        li, bp, bc = lays.u8(), int(rng.choice(BASES)), int(rng.choice(BASES))
        for slack in (0, 37):
            def body(run, short=0, slack=slack):
                a = run.inp("src", frame.reshape(1, H, 3 * W), li, device="cpu")
                p = run.out("packet", 1, len(want_pkt) + slack - (short == 1), 1, Layout(bp), device="cpu")
                c = run.out("config", 1, len(want_cfg) + slack - (short == 2), 1, Layout(bc), device="cpu")
                ps, cs = C.c_size_t(), C.c_size_t()
                rc = L.mdvt_ffv1_encode_frame(W, H, slices[0], slices[1], a.ptr, a.pitch, k % 2, 1, p.ptr, p.row_bytes, C.byref(ps),
                                              c.ptr, c.row_bytes, C.byref(cs))
                run.sizes = (ps.value, cs.value)
                return rc
            res = []
            for comp in (False, True):
                run = Run(entry, comp, k, "cpu")
                assert body(run) == 0
                out = run.check()
                assert run.sizes == (len(want_pkt), len(want_cfg))
                res.append((out["packet"].reshape(-1)[:run.sizes[0]].tobytes(), out["config"].reshape(-1)[:run.sizes[1]].tobytes(),
                            out["packet"].reshape(-1)[run.sizes[0]:].tobytes(), out["config"].reshape(-1)[run.sizes[1]:].tobytes()))
                # bytes of the capacity behind the packet / the record stay as they were
                assert res[-1][2] == run.arenas["packet"].payload(run.arenas["packet"].poison).reshape(-1)[run.sizes[0]:].tobytes()
                assert res[-1][3] == run.arenas["config"].payload(run.arenas["config"].poison).reshape(-1)[run.sizes[1]:].tobytes()
            assert res[0][:2] == res[1][:2] == (want_pkt, want_cfg)
            accepted(entry, arenas=list(run.arenas.values()))
        back = ffv1_ref.decode_frame_v3(want_pkt, ffv1_ref.parse_config_record(want_cfg), W, H)       # RGB, whatever the source order
        assert np.array_equal(back[..., ::-1] if k % 2 else back, frame[0]), (W, H, slices, k)
        refused(entry, lambda run: body(run, short=1, slack=0), -1, seed=k, device="cpu")     # packet_cap one byte short
    finish_entry(entry)
