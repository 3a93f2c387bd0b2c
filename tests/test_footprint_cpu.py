"""No GPU needed: the arena of tests/footprint.py catches what it is there to catch (on host tensors), and the list of entry points
the footprint tests cover is in step with include/mdvt.h -- a new entry point that writes through a pointer needs a footprint case
(or a commented exemption) before this passes."""
import os

import numpy as np
import pytest

import footprint as fp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_writing_entry_point_of_the_header_has_a_footprint_case():
    decls = fp.header_entry_points(os.path.join(REPO, "include", "mdvt.h"))
    assert len(decls) >= 30 and "mdvt_render_stereo" in decls and "mdvt_encode_video_frames" in decls
    writers = {n for n, args in decls.items() if fp.writes_through_a_pointer(args)}
    missing = sorted(writers - set(fp.ENTRY_POINTS) - set(fp.EXEMPT))
    assert not missing, f"entry points that write through a pointer without a footprint case or an exemption: {missing}"
    # the render calls and the in-place fill take their buffers through a const struct / a plain pointer: named here by hand
    for name in ("mdvt_render_stereo", "mdvt_render_stereo_batch", "mdvt_infill_using_mask_normals"):
        assert name in fp.ENTRY_POINTS
    stale = sorted((set(fp.ENTRY_POINTS) | set(fp.EXEMPT)) - set(decls))
    assert not stale, f"listed in tests/footprint.py but not declared in include/mdvt.h: {stale}"
    assert not set(fp.ENTRY_POINTS) & set(fp.EXEMPT)
    # the GPU test file has a test that tallies under each name (`entry = "<name>"` or a finish_entry / _finish_cases call with it),
    # and its last test insists that every name is in the table when the whole file ran
    src = open(os.path.join(REPO, "tests", "test_gpu_footprint.py")).read()
    code = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith(("#", '"""')))
    for name in fp.ENTRY_POINTS:
        assert (f'entry = "{name}"' in code or f'finish_entry("{name}"' in code or f'_finish_cases(mods, orc, "{name}"' in code), \
            f"tests/test_gpu_footprint.py has no case family for {name}"
    video = fp.header_entry_points(os.path.join(REPO, "include", "mdvt_video.h"))
    assert set(fp.HOST_VIDEO_ENTRY_POINTS) <= set(video)


def test_ffv1_encode_frame_footprint_on_the_host():
    """The host encoder's packet and configuration buffers of a stated capacity (include/mdvt_video.h): exact, generous, one byte short."""
    pytest.importorskip("torch")
    fp.ffv1_encode_frame_cases()


def test_the_parser_sees_pointer_arguments():
    assert fp.writes_through_a_pointer("mdvt_ctx* ctx, const uint8_t* d_rgb, size_t rgb_pitch, float* d_depth, void* stream")
    assert not fp.writes_through_a_pointer("mdvt_ctx* ctx, const mdvt_config* cfg")
    assert not fp.writes_through_a_pointer("mdvt_ctx* ctx, const uint8_t* a, void* stream")
    assert fp.writes_through_a_pointer("int width, int height, double fov, float* h_map_x, float* h_map_y")


@pytest.mark.parametrize("base", [0, 1, 3, 12])
@pytest.mark.parametrize("complement", [False, True])
def test_arena_layout_and_poison(base, complement):
    pytest.importorskip("torch")
    a = fp.Arena(3, 10, 13, n_frames=2, stride=50, base_offset=base, seed=5, complement=complement, device="cpu", name="t")
    assert a.ptr % 256 == base and a.guard >= 4096 and a.start >= a.guard
    assert a.inside.sum() == 2 * 3 * 10 and a.changed().size == 0
    other = fp.Arena(3, 10, 13, n_frames=2, stride=50, base_offset=base, seed=5, complement=not complement, device="cpu")
    lo, hi = a.start - a.guard, a.start + a.span + a.guard
    assert np.array_equal(a.poison[lo:hi], ~other.poison[other.start - other.guard:other.start + other.span + other.guard])
    assert 20 < len(np.unique(a.poison)) <= 256                  # not a constant
    data = np.arange(60, dtype=np.uint8).reshape(2, 3, 10)
    a.write(data)
    assert np.array_equal(a.payload(), data) and a.changed().size == 0
    # one byte past a row's end, one in the gap between the frames, one before the first row, one after the last
    for off, text in ((a.start + 13 + 10, "(frame 0, row 1, byte 10) = pitch padding, 0 bytes past"), (a.start + 45, "gap after frame 0, byte 6"),
                      (a.start - 1, "guard before the payload, 1 bytes"), (a.start + a.span, "guard after the payload, 0 bytes")):
        a.buf[off] ^= 0x40
        offs = a.changed()
        assert list(offs) == [off] and text in a.report(a.read(), offs), a.report(a.read(), offs)
        a.buf[off] ^= 0x40
    a.buf[a.start + 3] ^= 1                                       # a payload byte is the call's to write
    assert a.changed().size == 0


def test_two_runs_catch_an_unwritten_byte_and_a_stray_one():
    pytest.importorskip("torch")
    def body(skip, stray):
        def run_body(run):
            src = run.inp("src", np.full((1, 4, 6), 9, np.uint8), fp.Layout(1, 3, 0))
            dst = run.out("dst", 4, 6, 1, fp.Layout(3, 1, 0))
            v = dst._view(dst.buf.numpy())
            v[...] = src.payload() + 1
            if skip:
                v[0, 2, 5] = dst.poison[dst.start + 2 * dst.pitch + 5]
            if stray:
                dst.buf[dst.start + 6] = 0x5A ^ dst.poison[dst.start + 6]
        return run_body
    out = fp.twice("unit", body(False, False), device="cpu")
    assert np.array_equal(out["dst"], np.full((1, 4, 6), 10, np.uint8))
    with pytest.raises(AssertionError, match=r"first at \(frame 0, row 2, byte 5\)"):
        fp.twice("unit", body(True, False), device="cpu")
    with pytest.raises(AssertionError, match=r"\(frame 0, row 0, byte 6\) = pitch padding, 0 bytes past the row's end"):
        fp.twice("unit", body(False, True), device="cpu")
