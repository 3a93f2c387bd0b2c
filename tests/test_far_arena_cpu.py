"""No GPU needed: the far arenas of tests/footprint.py catch what they are there to catch.  The same window and alias bookkeeping as
on the device, with host bytes for the windows only (fp.HostSlab), and a modelled kernel that copies every row of a batch from a
source lane to a destination lane at the addresses it computes -- correctly, and with each 32-bit slip of fp.SLIPS in its stores or
in its loads.  For every layout tests/test_gpu_far_offsets.py uses:

  1. every modelled access lies inside the slab, in a watched window (so on the device a slip cannot fault);
  2. the correct kernel passes the checker;
  3. every slip that changes an address on that layout is flagged, by changed() or by a payload that is not the expected one;
  4. no window of an alias overlaps a payload (recomputed here by brute force, not with the arena's own search).

The second half keeps fp.FAR_CASES in step with the three headers."""
import os
import re

import numpy as np
import pytest

import footprint as fp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VEC, ODD = fp.Layout(4, 4, 4), fp.Layout(1, 3, 1)

# name: (Far keywords, frames, rows, layout)
LAYOUTS = {
    "far stride, vector": (dict(kind="stride"), 3, 11, VEC),
    "far stride, bytes": (dict(kind="stride"), 3, 9, ODD),
    "far stride, separate eyes far apart": (dict(kind="stride", apart=("right_",)), 3, 11, VEC),
    "far stride, 8 frames a quarter of 2^32 apart": (dict(kind="stride", stride_unit=1 << 30), 8, 11, ODD),
    "far stride, 9 frames a quarter of 2^32 apart, vector": (dict(kind="stride", stride_unit=1 << 30), 9, 9, VEC),
    "far pitch, one frame, vector": (dict(kind="pitch"), 1, 11, VEC),
    "far pitch, one frame, bytes": (dict(kind="pitch"), 1, 11, ODD),
    "far pitch, two frames, vector": (dict(kind="pitch"), 2, 9, VEC),
    "far pitch, two frames, bytes": (dict(kind="pitch"), 2, 9, ODD),
    "far pitch of the input alone": (dict(kind="pitch", only=("src",)), 1, 9, ODD),
    "far base alone": (dict(kind="near", apart=("dst", "right_")), 3, 9, ODD),
    "pitch 2^24 - 1, 256 rows (the marches' last accepted plane)": (dict(kind="pitch", pitch=(1 << 24) - 1), 1, 256, ODD),
}


def _lanes(run, N, H, W, lay, rng):
    src = rng.integers(0, 256, (N, H, 3 * W), dtype=np.uint8)           # every frame and row its own content
    return (run.inp("src", src, lay), run.out("dst", H, 3 * W, N, lay), run.out("right_dst", H, 3 * W, N, fp.Layout((lay.base + 8) % 16, lay.pad, lay.gap)),
            run.out("planes", H, 4 * W, N, fp.Layout(0, 16, 16) if lay is VEC else fp.Layout(0, 4, 4)), src)


def _model(slab, src, dsts, load_slip=None, store_slip=None):
    """dst(f, row) := src(f, row) + 1 for every destination lane, addresses as the slips give them."""
    right = lambda f, r, s, p: f * s + r * p
    for f in range(src.n_frames):
        for r in range(src.rows):
            row = slab.load(src.origin + (load_slip or right)(f, r, src.stride, src.pitch), src.row_bytes)
            for d in dsts:
                slab.store(d.origin + (store_slip or right)(f, r, d.stride, d.pitch), np.resize(row + 1, d.row_bytes))


def _flagged(run, want):
    """What Run.check and the test's comparison would object to."""
    found = []
    for name, a in run.arenas.items():
        host = a.read()
        offs = a.changed(host)
        if offs.size:
            found.append(a.report(host, offs, limit=1))
        pay = a.payload(host)
        if a.input is not None and not np.array_equal(pay, a.input):
            found.append(f"{name}: input changed")
        if a.input is None and not np.array_equal(pay, want[name]):
            found.append(f"{name}: payload is not the expected one")
    return found


def _moves(slip, a):
    return any(slip(f, r, a.stride, a.pitch) != f * a.stride + r * a.pitch for f in range(a.n_frames) for r in range(a.rows))


# the slips each kind of layout must be able to show (test_every_modelled_slip_is_flagged insists that they moved an address there)
FRAME_SLIPS = {"frame term truncated", "sum truncated", "frame term sign-extended", "sum sign-extended", "frame term by 24-bit multiply",
               "both terms by 24-bit multiply"}
ROW_SLIPS = {"row term truncated", "sum truncated", "row term sign-extended", "sum sign-extended", "row term by 24-bit multiply",
             "both terms by 24-bit multiply"}
CASES = [(name, W) for name in sorted(LAYOUTS) for W in ((36, 64) if LAYOUTS[name][3] is VEC else (33,) if LAYOUTS[name][2] == 256 else (33, 37))]


@pytest.mark.parametrize("layout,W", CASES)
def test_every_modelled_slip_is_flagged(layout, W):
    kw, N, H, lay = LAYOUTS[layout]
    rng = np.random.default_rng(W + N)
    cases = [(None, None, "correct")] + [(None, s, k) for k, s in fp.SLIPS.items()] + [(s, None, k) for k, s in fp.SLIPS.items()]
    shown = set()
    for load_slip, store_slip, what in cases:
        for complement in ((False, True) if what == "correct" else (bool(len(what) % 2),)):
            slab = fp.HostSlab()
            run = fp.FarRun("model", complement, 7, "cpu", fp.Far(slab, **kw))
            src, dst, right, planes, data = _lanes(run, N, H, W, lay, rng)
            assert max(a.iv_end.max() for a in run.arenas.values()) <= slab.size <= 12 << 30
            dsts = (dst, right, planes)
            want = {"dst": data + 1, "right_dst": data + 1, "planes": np.stack([[np.resize(r + 1, 4 * W) for r in fr] for fr in data])}
            if what == "correct":
                # 4. brute force: the windows of aliases against every payload row of every lane
                for a in run.arenas.values():
                    ws, we, true = a.win
                    for b in run.arenas.values():
                        rows = b.pay_starts
                        sel = ~true if a is b else np.ones(true.size, bool)
                        over = (ws[sel][:, None] < rows[None, :] + b.row_bytes) & (rows[None, :] < we[sel][:, None])
                        assert not over.any(), (layout, a.name, b.name)
            _model(slab, src, dsts, load_slip, store_slip)
            # 1. inside the slab, in a watched window
            assert not slab.outside, (layout, what, slab.outside[:3])
            assert not slab.unwatched, (layout, what, slab.unwatched[:3])
            found = _flagged(run, want)
            moved = (load_slip and _moves(load_slip, src)) or (store_slip and any(_moves(store_slip, d) for d in dsts))
            if not moved:
                assert not found, (layout, what, found)                                   # 2. (and slips this layout cannot show)
                run.check()
            else:
                assert found, f"{layout}, W = {W}: the slip '{what}' in the {'stores' if store_slip else 'loads'} goes unnoticed"       # 3.
                if store_slip:
                    assert any("changed in the lane's windows" in t for t in found), (layout, what, found)
                    with pytest.raises(AssertionError):
                        run.check()
                shown.add(what)
    if kw["kind"] == "stride":
        assert FRAME_SLIPS <= shown, (layout, sorted(FRAME_SLIPS - shown))
    if kw["kind"] == "pitch" and not kw.get("pitch"):
        assert ROW_SLIPS <= shown, (layout, sorted(ROW_SLIPS - shown))
        if N > 1:
            assert set(fp.SLIPS) <= shown, (layout, sorted(set(fp.SLIPS) - shown))


def test_the_three_layouts_cross_both_boundaries():
    p, s, _ = fp.Far(None, "stride").place("x", 11, 192, 3, VEC)
    assert s > 1 << 31 and s % 4 == 0 and s - (1 << 31) < 1 << 16 and 2 * s > 1 << 32
    p, s, _ = fp.Far(None, "stride").place("x", 11, 4 * 64, 3, fp.Layout(0, 16, 16))
    assert s % 16 == 0 and p % 16 == 0
    p, s, _ = fp.Far(None, "stride").place("x", 9, 99, 3, ODD)
    assert s % 2 == 1
    p, s, _ = fp.Far(None, "pitch").place("x", 9, 99, 2, ODD)
    assert p > 1 << 29 and p % 2 == 1 and p - (1 << 29) < 1 << 16 and 4 * p > 1 << 31 and 8 * p > 1 << 32 and s >= 9 * p
    p, s, _ = fp.Far(None, "pitch").place("x", 9, 192, 2, VEC)
    assert p % 4 == 0 and s % 4 == 0
    p, s, _ = fp.Far(None, "stride", stride_unit=1 << 30).place("x", 9, 99, 8, ODD)
    assert 2 * s > 1 << 31 and 4 * s > 1 << 32 and fp.SLAB_FRONT + 8 * s < fp.SLAB_BYTES
    assert fp.Far(None, "near", apart=("right_",)).place("right_rgb", 9, 99, 3, ODD)[2] > 1 << 32
    assert fp.SLAB_FRONT >= (1 << 31) + fp.GUARD and fp.SLAB_BYTES <= 12 << 30


def test_a_slip_is_reported_with_its_lane_and_alias():
    slab = fp.HostSlab()
    run = fp.FarRun("model", False, 3, "cpu", fp.Far(slab, "stride"))
    dst = run.out("dst", 9, 99, 3, ODD)
    slab.store(dst.origin + fp.t32(2 * dst.stride) + 4 * dst.pitch, np.full(99, 7, np.uint8))
    with pytest.raises(AssertionError, match=r"model dst .*far stride.*\n.*byte 0 of \[frame trunc \+ row true\] of \(frame 2, row 4\)"):
        run.check()


# ------------------------------------------------------------------------------------------------------------- the headers
def test_every_entry_point_with_a_pitch_stride_or_offset_has_far_cases():
    decls = {}
    for h in ("mdvt.h", "mdvt_ffv1_decode.h", "mdvt_convergence.h"):
        decls.update(fp.header_entry_points(os.path.join(REPO, "include", h)))
    assert "mdvt_decode_video_frames" in decls and "mdvt_convergence_depths" in decls and len(decls) >= 32
    need = {n for n, args in decls.items() if fp.takes_far_arguments(args)}
    assert {"mdvt_swap_rb", "mdvt_decode_depth", "mdvt_encode_video_frames", "mdvt_decode_video_frames", "mdvt_convergence_depths"} <= need
    # the render calls take their pitches and strides in a const struct: named by hand
    need |= {"mdvt_render_stereo", "mdvt_render_stereo_batch"}
    missing = sorted(need - set(fp.FAR_CASES))
    assert not missing, f"entry points with a pitch, a stride or a 64-bit offset or capacity, without an entry in fp.FAR_CASES: {missing}"
    stale = sorted(set(fp.FAR_CASES) - set(decls) - set(fp.FAR_LIBRARY_BLOCKS))
    assert not stale, f"in fp.FAR_CASES but not declared in a header: {stale}"
    src = open(os.path.join(REPO, "tests", "test_gpu_far_offsets.py")).read()
    tests = set(re.findall(r"^def (test_\w+)\(", src, flags=re.M))
    for name, case in fp.FAR_CASES.items():
        if isinstance(case, str):
            assert len(case) > 20 and "\n" not in case, f"{name}: a reason is one line"
            continue
        assert case, name
        for kind, where in case.items():
            assert kind in ("stride", "pitch", "base", "refused", "offsets", "block"), (name, kind)
            named = [w for w in where.split() if w.startswith("test_")]
            assert named or len(where) > 20, f"{name} {kind}: name the tests, or say in a line why the layout cannot apply"
            for t in named:
                assert t.rstrip(",;") in tests, f"{name} {kind}: tests/test_gpu_far_offsets.py has no {t}"


def test_the_parser_sees_far_arguments():
    assert fp.takes_far_arguments("mdvt_ctx* ctx, const uint8_t* d_rgb, size_t rgb_pitch, float* d_depth, void* stream")
    assert fp.takes_far_arguments("mdvt_ctx* ctx, const uint8_t* d, size_t frame_stride")
    assert fp.takes_far_arguments("const uint8_t* d_packets, uint64_t packets_bytes, const uint64_t* d_offsets")
    assert fp.takes_far_arguments("uint8_t* d_packets, uint64_t packets_cap")
    assert fp.takes_far_arguments("int what, void* h_dst, uint64_t capacity, uint64_t info[8]")
    assert not fp.takes_far_arguments("mdvt_ctx* ctx, int which, uint64_t seed, uint64_t* h_mismatches")
    assert not fp.takes_far_arguments("const uint8_t* h_config, size_t config_size")
