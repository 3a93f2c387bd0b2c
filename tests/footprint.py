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


def takes_far_arguments(args):
    """True if an argument list has a size_t pitch or stride, or a uint64_t offset or capacity (by value or as an array)."""
    return bool(re.search(r"\bsize_t\s+\w*(pitch|stride)\b", args) or
                re.search(r"\buint64_t\s*\*?\s*\w*(offsets?|cap|capacity|packets_bytes)\b", args))


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
        run = new_run(entry, comp, seed, device)
        body(run)
        res.append(run.check())
    compare_runs(entry, res[0], res[1], what)
    LAST_RUN = list(run.arenas.values())
    return res[0]


def refused(entry, body, status, seed=1, device="cuda"):
    """A layout the ABI refuses: body(run) returns the status of the call; every arena must be as it was."""
    for comp in (False, True):
        run = new_run(entry, comp, seed, device)
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


# ---------------------------------------------------------------------------------------------------------------- far layouts
# Frames and rows more than 4 GiB apart.  The ABI takes pitches and strides as size_t, so a caller may put tiny frames gigabytes
# apart; a kernel that computes `f * stride + row * pitch` in 32 bits then reads or writes somewhere else.  All buffers of a call
# are *lanes* of one *slab* (one uint8 tensor per test module, never filled as a whole), and for every lane every address a 32-bit
# slip could compute -- each term or the sum truncated, sign-extended, or multiplied in 24 bits -- lies inside the slab in a poisoned,
# watched window: a slip shows as a changed poison byte or a wrong payload, never as a fault.  tests/test_far_arena_cpu.py proves that
# on modelled kernels; tests/test_gpu_far_offsets.py runs the entry points.

FAR_STRIDE, FAR_PITCH = 1 << 31, 1 << 29          # + a small delta per lane kind: the far stride and the far pitch
FAR_BASE = (1 << 32) + (1 << 21)                  # what separates the buffers of a far-base layout
SLAB_BYTES = 11 << 30                             # (the two-frame far pitch at H = 9 needs about 10.6 GiB)
SLAB_FRONT = (1 << 31) + (1 << 22)                # margin before the first lane: a negative 32-bit offset stays inside
SLAB_LANE = 1 << 22                               # sub-offset between two lanes
SLAB_SKIP = "less than twice the slab is free on the device"


def t32(v):
    return v & 0xFFFFFFFF


def s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def m24(a, b):
    """__umul24: the low 32 bits of the product of the low 24 bits."""
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & 0xFFFFFFFF


TERM = {"true": lambda a, b: a * b, "trunc": lambda a, b: t32(a * b), "sext": lambda a, b: s32(a * b), "mul24": m24}

# the offset a kernel with one slip computes for (frame f, row r); "correct" is f * stride + r * pitch in 64 bits
SLIPS = {
    "frame term truncated": lambda f, r, s, p: t32(f * s) + r * p,
    "row term truncated": lambda f, r, s, p: f * s + t32(r * p),
    "sum truncated": lambda f, r, s, p: t32(f * s + r * p),
    "frame term sign-extended": lambda f, r, s, p: s32(f * s) + r * p,
    "row term sign-extended": lambda f, r, s, p: f * s + s32(r * p),
    "sum sign-extended": lambda f, r, s, p: s32(f * s + r * p),
    "frame term by 24-bit multiply": lambda f, r, s, p: m24(f, s) + r * p,
    "row term by 24-bit multiply": lambda f, r, s, p: f * s + m24(r, p),
    "both terms by 24-bit multiply": lambda f, r, s, p: m24(f, s) + m24(r, p),
}


def alias_offsets(n_frames, rows, stride, pitch):
    """-> [(f, row, class, offset)]: every offset a 32-bit slip could compute for a row -- each variant of the frame term with each
    variant of the row term, and the truncated and the sign-extended sum.  The class "frame true + row true" is the row itself."""
    res = []
    for f in range(n_frames):
        fv = [(k, fn(f, stride)) for k, fn in TERM.items()]
        for r in range(rows):
            for kf, vf in fv:
                for kr, fn in TERM.items():
                    res.append((f, r, f"frame {kf} + row {kr}", vf + fn(r, pitch)))
            res.append((f, r, "sum trunc", t32(f * stride + r * pitch)))
            res.append((f, r, "sum sext", s32(f * stride + r * pitch)))
    return res


def _poison_at(offs, seed, complement):
    """The poison of the slab's bytes at `offs` (uint64): a hash of (seed, offset), so that windows of two lanes that overlap agree."""
    x = offs.astype(np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15 + 0x6d647674) & 0xFFFFFFFFFFFFFFFF)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    p = ((x >> np.uint64(33)) & np.uint64(0xFF)).astype(np.uint8)
    return ~p if complement else p


class Slab:
    """The device slab: `size` bytes from a 256-byte boundary, allocated once and never touched as a whole."""
    host = False

    def __init__(self, size=SLAB_BYTES, device="cuda"):
        import torch
        self.size, self.device = int(size), device
        self.buf = torch.empty(self.size + 256, dtype=torch.uint8, device=device)
        self.base = -self.buf.data_ptr() % 256
        self.lanes = []

    @staticmethod
    def skip_reason(size=SLAB_BYTES):
        """The one permitted skip: None if twice the slab is free on the device."""
        import torch
        free, _ = torch.cuda.mem_get_info()
        return None if free >= 2 * size else SLAB_SKIP

    def ptr(self, off):
        return self.buf.data_ptr() + self.base + int(off)

    def put(self, starts, lens, data):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(data)).to(self.device)
        pos = 0
        for s, n in zip(starts.tolist(), lens.tolist()):
            self.buf[self.base + s: self.base + s + n].copy_(t[pos:pos + n])
            pos += n

    def get(self, starts, lens):
        import torch
        return torch.cat([self.buf[self.base + s: self.base + s + n] for s, n in zip(starts.tolist(), lens.tolist())]).cpu().numpy()


class HostSlab:
    """The slab's bookkeeping without its memory (no GPU): host bytes for the watched windows only, in 4 KiB pages.  store() is what a
    modelled kernel writes with; a store outside [0, size) or into a page no window touches is recorded, not made."""
    host, PAGE = True, 4096

    def __init__(self, size=SLAB_BYTES):
        self.size, self.pages, self.lanes = int(size), {}, []
        self.outside, self.unwatched = [], []

    def ptr(self, off):
        return int(off)                                   # (addresses are slab offsets)

    def _pieces(self, s, n):
        while n > 0:
            page, o = divmod(s, self.PAGE)
            k = min(n, self.PAGE - o)
            yield page, o, k
            s, n = s + k, n - k

    def put(self, starts, lens, data):
        pos = 0
        for s, n in zip(starts.tolist(), lens.tolist()):
            for page, o, k in self._pieces(s, n):
                self.pages.setdefault(page, np.zeros(self.PAGE, np.uint8))[o:o + k] = data[pos:pos + k]
                pos += k

    def get(self, starts, lens):
        out = np.empty(int(lens.sum()), np.uint8)
        pos = 0
        for s, n in zip(starts.tolist(), lens.tolist()):
            for page, o, k in self._pieces(s, n):
                out[pos:pos + k] = self.pages[page][o:o + k]
                pos += k
        return out

    def load(self, off, n):
        off, out = int(off), np.zeros(int(n), np.uint8)
        if off < 0 or off + n > self.size:
            self.outside.append(off)
            return out
        pos = 0
        for page, o, k in self._pieces(off, n):
            if page in self.pages:
                out[pos:pos + k] = self.pages[page][o:o + k]
            else:
                self.unwatched.append(off + pos)
            pos += k
        return out

    def store(self, off, data):
        off, data = int(off), np.asarray(data, np.uint8)
        if off < 0 or off + data.size > self.size:
            self.outside.append(off)
            return
        pos = 0
        for page, o, k in self._pieces(off, data.size):
            if page in self.pages:
                self.pages[page][o:o + k] = data[pos:pos + k]
            else:
                self.unwatched.append(off + pos)
            pos += k


def _hits(ws, we, starts, row_bytes):
    """Indices of the windows [ws, we) that overlap a payload row [s, s + row_bytes) of the sorted `starts`."""
    i = np.searchsorted(starts, ws - row_bytes, side="right")
    ok = i < starts.size
    return np.flatnonzero(ok & (starts[np.minimum(i, starts.size - 1)] < we))


class FarArena(Arena):
    """Arena's interface on a lane of a slab: only the windows are poisoned and read back.  `host` arrays (read(), poison, inside)
    are the windows' bytes one after the other, in the order of their addresses."""

    def __init__(self, slab, lane, rows, row_bytes, pitch=None, n_frames=1, stride=None, base_offset=0, guard=GUARD, *, seed=0,
                 complement=False, name="", far_base=0, strict=True):
        self.slab, self.lane = slab, int(lane)
        self.rows, self.row_bytes, self.n_frames = int(rows), int(row_bytes), int(n_frames)
        self.pitch = int(row_bytes if pitch is None else pitch)
        self.stride = int(self.rows * self.pitch if stride is None else stride)
        assert self.rows >= 1 and self.row_bytes >= 1 and self.n_frames >= 1
        assert self.pitch >= self.row_bytes and self.stride >= self.rows * self.pitch and 0 <= base_offset < 16
        # at least GUARD and at least two rows (of a far pitch: two rows' bytes) around everything a row's address could be
        self.guard = max(int(guard), GUARD, 2 * (self.pitch if self.pitch < (1 << 20) else self.row_bytes))
        self.base_offset, self.name, self.complement = int(base_offset), name, bool(complement)
        self.span = (self.n_frames - 1) * self.stride + self.rows * self.pitch
        self.origin = SLAB_FRONT + self.lane * SLAB_LANE + int(far_base) + self.base_offset       # slab offset of the payload's first byte
        al = alias_offsets(self.n_frames, self.rows, self.stride, self.pitch)
        self.alias = al
        off = np.array([a[3] for a in al], np.int64) + self.origin
        true = np.array([a[3] == a[0] * self.stride + a[1] * self.pitch for a in al])
        ws, we = off - self.guard, off + self.row_bytes + self.guard
        assert ws.min() >= 0 and we.max() <= slab.size, (f"{name}: an address a 32-bit slip could compute lies outside the slab "
                                                          f"([{ws.min()}, {we.max()}) of {slab.size})")
        self.alias_at = off
        self.pay_starts = np.unique(off[true])
        self.win = (ws, we, true)
        # no window of an alias may lie on a payload (its own lane's or another's), and no window at all on another lane's
        # (strict=False, for a layout the call must refuse: an alias may fall on the lane's own rows -- at a pitch of 2^24 the 24-bit
        # product is 0 -- which is still inside the slab)
        bad = _hits(ws[~true], we[~true], self.pay_starts, self.row_bytes) if strict else np.zeros(0, np.int64)
        assert bad.size == 0, f"{name}: the window of alias '{[a for a, t in zip(al, true) if not t][bad[0]]}' overlaps the lane's own payload"
        for o in slab.lanes:
            assert _hits(ws, we, o.pay_starts, o.row_bytes).size == 0, f"{name}: a window overlaps the payload of {o.name}"
            assert _hits(o.win[0], o.win[1], self.pay_starts, self.row_bytes).size == 0, f"{o.name}: a window overlaps the payload of {name}"
        slab.lanes.append(self)
        # the windows, merged
        order = np.argsort(ws, kind="stable")
        s, e = ws[order], np.maximum.accumulate(we[order])
        first = np.ones(s.size, bool)
        first[1:] = s[1:] > e[:-1]
        self.iv_start = s[first]
        self.iv_end = np.append(e[:-1][first[1:]], e[-1])
        self.iv_len = self.iv_end - self.iv_start
        self.iv_pos = np.concatenate([[0], np.cumsum(self.iv_len)[:-1]])
        total = int(self.iv_len.sum())
        rows_at = self.origin + (np.arange(self.n_frames)[:, None] * self.stride + np.arange(self.rows)[None, :] * self.pitch)
        self.pay_index = self._pos(rows_at)[..., None] + np.arange(self.row_bytes)
        self.abs = np.repeat(self.iv_start - self.iv_pos, self.iv_len) + np.arange(total)            # slab offset of every host byte
        self.poison = _poison_at(self.abs, seed, self.complement)
        self.inside = np.zeros(total, bool)
        self.inside[self.pay_index] = True
        self.input, self.inout = None, False
        slab.put(self.iv_start, self.iv_len, self.poison)

    def _pos(self, at):
        """Slab offsets inside the windows -> positions in the host arrays."""
        i = np.searchsorted(self.iv_start, at, side="right") - 1
        return self.iv_pos[i] + (at - self.iv_start[i])

    @property
    def ptr(self):
        return self.slab.ptr(self.origin)

    def write(self, data, inout=False):
        d = np.ascontiguousarray(data).view(np.uint8).reshape(self.n_frames, self.rows, self.row_bytes)
        host = self.poison.copy()
        host[self.pay_index] = d
        self.slab.put(self.iv_start, self.iv_len, host)
        self.input, self.inout = d.copy(), bool(inout)
        return self

    def read(self):
        return self.slab.get(self.iv_start, self.iv_len)

    def payload(self, host=None, dtype=np.uint8):
        host = self.read() if host is None else host
        return np.ascontiguousarray(host[self.pay_index]).view(dtype)

    def where(self, pos):
        rel = int(self.abs[int(pos)]) - self.origin
        b = rel + self.origin - self.alias_at                                # the byte's position in every alias row
        near = np.where(b < 0, -b, np.maximum(0, b - self.row_bytes + 1))
        names = []
        for i in np.argsort(near, kind="stable")[:3]:
            if near[i] > self.guard:
                break
            f, r, cls, _ = self.alias[i]
            bi = int(b[i])
            side = f"{-bi} bytes before" if bi < 0 else f"byte {bi} of" if bi < self.row_bytes else f"{bi - self.row_bytes} bytes past"
            names.append(f"{side} [{cls}] of (frame {f}, row {r})")
        return f"offset {rel:+d} from the lane's pointer: " + "; ".join(names)

    def report(self, host, offs, limit=6):
        return Arena.report(self, host, offs, limit).replace("outside the payload changed", "outside the payload changed in the lane's windows", 1)


class Far:
    """How a run lays its buffers out on the slab.  kind "stride": frames FAR_STRIDE + delta apart (stride_unit replaces FAR_STRIDE
    for a long batch); "pitch": rows FAR_PITCH + delta apart (or exactly `pitch` apart: the boundary of a documented limit), frames
    behind each other; "near": neither.  only: the names of the buffers that go far (default: all).  apart: name prefixes of the
    buffers that lie FAR_BASE behind the others (the far-base layout)."""

    def __init__(self, slab, kind, only=None, apart=(), stride_unit=FAR_STRIDE, pitch=None, refusal=False):
        assert kind in ("stride", "pitch", "near")
        self.slab, self.kind, self.only, self.apart, self.stride_unit, self.pitch = slab, kind, only, tuple(apart), int(stride_unit), pitch
        self.refusal = bool(refusal)                 # the layout is one the call must refuse (FarArena's strict=False)

    @staticmethod
    def delta(need, like):
        """The window's size rounded up to a multiple of 16, plus `like` % 16: a far pitch keeps the alignment of the layout's row
        padding, a far stride that of its gap -- odd on the byte-path layouts, a multiple of 4 or 16 where the vector paths want one
        (and the same for the two eyes' buffers, which share one pitch and one stride)."""
        return -(-need // 16) * 16 + like % 16

    def place(self, name, rows, row_bytes, n_frames, lay):
        """-> pitch, stride, bytes behind the lane's sub-offset"""
        far = self.only is None or name in self.only
        pitch = row_bytes + lay.pad
        if self.kind == "pitch" and far and rows > 1:
            pitch = int(self.pitch) if self.pitch else FAR_PITCH + self.delta(row_bytes + 2 * max(GUARD, 2 * row_bytes), lay.pad)
        stride = rows * pitch + lay.gap
        if self.kind == "stride" and far and n_frames > 1:
            stride = self.stride_unit + self.delta(rows * pitch + 2 * max(GUARD, 2 * pitch), lay.gap)
        return pitch, stride, FAR_BASE if name.startswith(self.apart) and self.apart else 0


class FarRun(Run):
    """Run whose device arenas are lanes of the far layout's slab (host arenas, e.g. lookup tables filled on the host, stay plain)."""

    def __init__(self, entry, complement, seed, device, far):
        Run.__init__(self, entry, complement, seed, device)
        self.far = far
        far.slab.lanes = []

    def _arena(self, name, rows, row_bytes, n_frames, lay, device=None):
        if (device or self.device) == "cpu" and not self.far.slab.host:
            return Run._arena(self, name, rows, row_bytes, n_frames, lay, device)
        lay = lay or Layout()
        pitch, stride, behind = self.far.place(name, rows, row_bytes, n_frames, lay)
        a = FarArena(self.far.slab, len(self.arenas), rows, row_bytes, pitch, n_frames, stride, lay.base, seed=self.seed,
                     complement=self.complement, name=f"{self.entry} {name} {lay} [far {self.far.kind}]", far_base=behind, strict=not self.far.refusal)
        a.lay = lay
        self.arenas[name] = a
        return a


FAR = None                                       # the far layout twice() and refused() build their runs on (far())


def new_run(entry, complement, seed, device):
    return Run(entry, complement, seed, device) if FAR is None else FarRun(entry, complement, seed, device, FAR)


class far:
    """with fp.far(Far(...)): twice() and refused() hand out far arenas, and the tally is the block's own."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        global FAR, TALLY
        self.saved = FAR, TALLY
        FAR, TALLY = self.mode, {}
        return self.mode

    def __exit__(self, *exc):
        global FAR, TALLY
        FAR, TALLY = self.saved
        return False


# Blocks the library owns that cross 4 GiB at sizes a test can afford (no argument of the ABI: named here, not found by the scan)
FAR_LIBRARY_BLOCKS = ("encoder scratch", "heap completion workspace", "general mesh key planes")

_NI_PLANE = ("the plane the march walks (include/mdvt.h: pitch below 2^24, pitch x height below 2^32) is refused at its boundary and "
             "beyond, test_march_plane_limits")

# every entry point with a size_t pitch or stride or a uint64_t offset or capacity (tests/test_far_arena_cpu.py holds the list to
# the headers) -> {layout: the tests of tests/test_gpu_far_offsets.py that run it there, or why the layout cannot apply}; a plain
# string: why no far layout applies to the entry point at all
FAR_CASES = {
    "mdvt_render_stereo": dict(pitch="test_render_single_far_pitch", stride="one frame per call: the strides are not read"),
    "mdvt_render_stereo_batch": dict(stride="test_render_batch_far_stride test_render_null_byte_masks_far_stride test_render_two_banks_far_stride",
                                     pitch="test_render_batch_far_pitch", base="test_render_batch_far_stride (separate eye buffers)"),
    "mdvt_decode_depth": dict(pitch="test_single_image_far_pitch"),
    "mdvt_encode_depth": dict(pitch="test_single_image_far_pitch"),
    "mdvt_touchly_depth": dict(pitch="test_single_image_far_pitch"),
    "mdvt_masked_blur": dict(pitch="test_single_image_far_pitch"),
    "mdvt_edge_filter": dict(pitch="test_single_image_far_pitch"),
    "mdvt_edge_point_pixels": dict(pitch="test_single_image_far_pitch"),
    "mdvt_infill_using_normals": dict(pitch="test_single_image_far_pitch (colour, normals, output)", refused=_NI_PLANE),
    "mdvt_mark_lower_side": dict(pitch="test_single_image_far_pitch (output)", refused=_NI_PLANE),
    "mdvt_equirect_remap": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch"),
    "mdvt_swap_rb": dict(stride="test_batched_far_stride (also in place)", pitch="test_batched_far_pitch"),
    "mdvt_finish_infill_mask": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch"),
    "mdvt_finish_infill_mask_stereo": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch", base="test_batched_far_stride"),
    "mdvt_finish_infill_mask_heap": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch"),
    "mdvt_finish_infill_mask_heap_stereo": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch", base="test_batched_far_stride"),
    "mdvt_normal_infill": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch (image, output)", refused=_NI_PLANE),
    "mdvt_infill_using_mask_normals": dict(stride="test_batched_far_stride", pitch="test_batched_far_pitch (image, mask image)", refused=_NI_PLANE),
    "mdvt_encode_video_frames": dict(stride="test_encode_video_frames_far_stride", block="test_encoder_scratch_block_past_4_gib",
                                     pitch="the slab holds one frame of far rows; the source rows are read as the far-stride frames are",
                                     offsets="packets follow each other without gaps: an offset past 2^32 needs 4 GiB of packets"),
    "mdvt_decode_video_frames": dict(stride="test_decode_video_frames_far", offsets="test_decode_video_frames_far (and packets_bytes one short)"),
    "mdvt_convergence_depths": dict(stride="test_convergence_depths_far", pitch="test_convergence_depths_far"),
    "mdvt_debug_read": "capacity is the size of a HOST buffer of the tuning library's diagnosis: nothing is addressed with it on the device",
    # library-owned blocks (FAR_LIBRARY_BLOCKS)
    "heap completion workspace": dict(block="test_heap_completion_workspace_past_4_gib"),
    "encoder scratch": dict(block="test_encoder_scratch_block_past_4_gib"),
    "general mesh key planes": "not covered: slots x npx x 8 B crosses 2^32 only from about 8K frames with 16 slots, which the oracle cannot afford in a test",
}
