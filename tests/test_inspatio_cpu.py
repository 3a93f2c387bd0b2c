"""The InSpatio-World alignment without a GPU: tests/inspatio_ref.py's two routes to the six integer sums agree, the sign and the
meaning of the shift hold on a known displacement (no scikit-image needed), the host's grid clean-up, frame padding and chunk
schedule (metric_depth_video_toolbox_amd/inspatio_world.py) give hand-made answers, and include/mdvt_inspatio.h is bound as declared."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import footprint as fp
import inspatio_ref as ir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")
HEADER = os.path.join(REPO, "include", "mdvt_inspatio.h")
NAMES = ["mdvt_flow_warp", "mdvt_inspatio_composite_eye", "mdvt_inspatio_model_frames", "mdvt_inspatio_prepare_eye", "mdvt_masked_shift_grid", "mdvt_masked_shift_path"]
F = np.float32


@pytest.fixture(scope="module")
def host():
    from metric_depth_video_toolbox_amd import inspatio_world
    return inspatio_world


# ---- the six sums: two routes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,fill", [(2, 2, 0.9), (5, 7, 0.5), (11, 23, 0.75), (12, 22, 0.3), (16, 9, 1.0)])
def test_the_two_routes_to_the_sums_agree_on_small_cells(h, w, fill):
    rng = np.random.default_rng(h * 100 + w)
    gI, gR = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    V = (rng.random((h, w)) < fill).astype(np.uint8) * 255
    direct = ir.sums_direct(gI, gR, V)
    by_fft, worst = ir.sums_fft(gI, gR, V)
    assert direct.shape == (6, 2 * h - 1, 2 * w - 1) and np.array_equal(direct, by_fft) and worst < 1e-6
    # the definition, term by term, at three displacements
    v = V != 0
    for dy, dx in ((0, 0), (1, -1), (-(h - 1), w - 1)):
        want = np.zeros(6, np.int64)
        for y in range(h):
            for x in range(w):
                yy, xx = y - dy, x - dx
                if 0 <= yy < h and 0 <= xx < w and v[y, x] and v[yy, xx]:
                    a, b = int(gI[y, x]), int(gR[yy, xx])
                    want += (1, a, b, a * b, a * a, b * b)
        assert direct[:, dy + h - 1, dx + w - 1].tolist() == want.tolist(), (dy, dx)


@pytest.mark.parametrize("what", ["noise", "all 255"])
def test_the_two_routes_agree_on_a_270_x_240_cell(what):
    """The float64 transform is exact with a wide margin at the size of a 1080p eye's cell: its largest distance from an integer
    stays far below the exactness threshold 0.5.  The direct sums are checked where they are cheap: on the closed forms of a fully
    valid constant cell, and on a band of displacements of the noise cell."""
    h, w = 270, 240
    rng = np.random.default_rng(270240)
    if what == "noise":
        gI, gR = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        V = (rng.random((h, w)) < 0.75).astype(np.uint8)
    else:
        gI = gR = np.full((h, w), 255, np.uint8)
        V = np.ones((h, w), np.uint8)
    by_fft, worst = ir.sums_fft(gI, gR, V)
    print(f"{what}: largest distance from an integer {worst:.3g}")
    assert worst < 1e-4
    if what == "all 255":
        oy = h - np.abs(np.arange(-(h - 1), h))
        ox = w - np.abs(np.arange(-(w - 1), w))
        N = oy[:, None] * ox[None, :]
        for k, scale in enumerate((1, 255, 255, 255 * 255, 255 * 255, 255 * 255)):
            assert np.array_equal(by_fft[k], N * scale)
    else:
        # the definition in integers at 40 displacements: the corners, the centre and random ones
        v = (V != 0).astype(np.int64)
        a, b = gI.astype(np.int64) * v, gR.astype(np.int64) * v
        ds = [(0, 0), (h - 1, w - 1), (-(h - 1), w - 1), (h - 1, -(w - 1)), (-(h - 1), -(w - 1)), (1, 0), (0, -1)]
        ds += [(int(rng.integers(-(h - 1), h)), int(rng.integers(-(w - 1), w))) for _ in range(33)]
        for dy, dx in ds:
            at = (slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx)))            # x
            to = (slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx)))          # x - d
            want = [int((x[at] * y[to]).sum()) for x, y in ((v, v), (a, v), (v, b), (a, b), (a * a, v), (v, b * b))]
            assert by_fft[:, dy + h - 1, dx + w - 1].tolist() == want, (dy, dx)


# ---- sign and meaning -----------------------------------------------------------------------------------------------------------------
def _shifted_scene(seed):
    """A 46 x 90 eye of uniform noise, about a quarter of it holes; the infilled frame shows the render from three rows further
    down: I[y] = R[y + 3] (the last rows repeat)."""
    rng = np.random.default_rng(seed)
    H, W = 46, 90
    V = np.full((H, W), 255, np.uint8)
    for _ in range(14):
        y, x = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 10))
        V[y:y + 8, x:x + 10] = 0
    R = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    R[V == 0] = 0
    I = np.concatenate([R[3:], np.repeat(R[-1:], 3, axis=0)], axis=0)
    return R, I, V


def test_sign_and_meaning_of_the_shift(host):
    R, I, V = _shifted_scene(7)
    assert 0.15 < (V == 0).mean() < 0.35
    for route in (ir.DIRECT, ir.TRANSFORM):
        shift, status = ir.shift_grid(R, I, V, route)
        assert status[:, 1:3].all()
        assert shift[:, 1:3].reshape(-1, 2).tolist() == [[3.0, 0.0]] * 8, "every interior cell: exactly (dy, dx) = (3, 0)"
    flow = host.clean_grid(shift, status)
    assert flow.dtype == np.float32 and np.array_equal(flow, np.broadcast_to(np.array([0, 3], F), (4, 4, 2))), flow
    out = ir.warp(I, flow)
    assert np.array_equal(out[3:], R[3:]), "the warp brings the render back outside a margin of three rows"
    # the other way round: the infilled frame shows the render from three rows further up
    I2 = np.concatenate([np.repeat(R[:1], 3, axis=0), R[:-3]], axis=0)
    shift2, status2 = ir.shift_grid(R, I2, V)
    assert shift2[:, 1:3].reshape(-1, 2).tolist() == [[-3.0, 0.0]] * 8


def test_ties_take_the_mean_and_a_flat_cell_gives_zero():
    # images of period 4 along x in a fully valid cell: the maxima at dx = 0 tie with none (the overlap shrinks with |dx|, and the
    # normalised correlation of an exact overlap is 1 at every multiple of 4 whose overlap keeps 0.3 of the pixels)
    h, w = 12, 24
    row = np.tile(np.array([10, 200, 90, 30], np.uint8), w // 4)
    g = np.repeat(row[None, :], h, axis=0)
    g = (g + np.arange(h, dtype=np.uint8)[:, None] * 3).astype(np.uint8)
    V = np.ones((h, w), np.uint8)
    got = ir.shift_2d(g, g, V)
    assert got == [0.0, 0.0]                                         # symmetric ties: the mean of -16 .. 16 in steps of 4
    sums = ir.sums_direct(g, g, V)
    assert ir.shift_of_sums(sums, (h - 1, w - 1)) == got == ir.shift_2d(g, g, V, ir.TRANSFORM)
    flat = np.full((h, w), 77, np.uint8)
    assert ir.shift_2d(flat, flat, V) == [0.0, 0.0]                  # den = 0 everywhere: c = 0 everywhere, the mean of all d
    assert str(ir.shift_2d(flat, flat, V)[0]) == "0.0"               # +0.0: the negation is the integer sum's


# ---- the clean-up ---------------------------------------------------------------------------------------------------------------------
def _grid(dy, dx):
    shift = np.zeros((4, 4, 2))
    shift[..., 0], shift[..., 1] = dy, dx
    return shift, np.ones((4, 4), np.uint8)


def test_clean_grid_removes_one_outlier(host):
    shift, status = _grid(2.0, -1.0)
    shift[1, 2] = (9.0, -1.0)
    flow = host.clean_grid(shift, status)
    assert np.array_equal(flow, np.broadcast_to(np.array([-1, 2], F), (4, 4, 2)))
    # beyond 20 pixels a cell is dropped before the MAD rule sees it
    shift[1, 2] = (2.0, 20.5)
    assert np.array_equal(host.clean_grid(shift, status), flow)
    shift[1, 2] = (2.0, -20.0)                                       # 20 itself stays, and is an outlier of the MAD rule
    assert np.array_equal(host.clean_grid(shift, status), flow)


def test_clean_grid_fills_an_unreliable_corner_from_its_three_neighbours(host):
    shift, status = _grid(0.0, 0.0)
    shift[..., 1] = np.arange(16).reshape(4, 4) * 0.25               # dx = 0, 0.25 .. 3.75: within 2 mad?  mad = 1.0, median 1.875
    status[0, 0] = 0
    flow = host.clean_grid(shift, status)
    vals = np.arange(16, dtype=F) * F(0.25)
    vals15 = vals[1:]
    med = F(np.median(vals15))
    mad = F(np.median(np.abs(vals15 - med))) + F(1e-8)
    keep = np.abs(vals - med) <= F(2) * mad
    keep[0] = False
    assert keep[[1, 4, 5]].all()
    want = (vals[1] + vals[4] + vals[5]) / F(3)
    assert flow[0, 0, 0] == want and flow[0, 0, 1] == 0
    assert flow[0, 1, 0] == vals[1] and flow[1, 1, 0] == vals[5]


def test_clean_grid_with_one_computed_cell_spreads_to_its_neighbours_only(host):
    shift, status = np.zeros((4, 4, 2)), np.zeros((4, 4), np.uint8)
    shift[2, 1], status[2, 1] = (4.0, -2.5), 1
    flow = host.clean_grid(shift, status)
    want = np.zeros((4, 4, 2), F)
    want[1:4, 0:3] = (-2.5, 4.0)                                     # the cell and its 8-neighbours; the MAD rule does not run
    assert np.array_equal(flow, want)
    assert np.array_equal(host.clean_grid(np.zeros((4, 4, 2)), np.zeros((4, 4), np.uint8)), np.zeros((4, 4, 2), F))


def test_flow_grids_average_with_the_previous_frame_that_has_one(host):
    shifts = np.zeros((4, 4, 4, 2))
    for i, dy in enumerate((1.0, 7.0, 2.0, 4.0)):
        shifts[i, ..., 0] = dy
    statuses = np.ones((4, 4, 4), np.uint8)
    grids, has = host.flow_grids(shifts, statuses, [5, 0, 9, 1])
    assert has.tolist() == [1, 0, 1, 1] and grids.dtype == np.float32
    assert np.all(grids[0, ..., 1] == 1.0) and np.all(grids[1] == 0)
    assert np.all(grids[2, ..., 1] == 2.0), "the frame before has no grid: its own alone"
    assert np.all(grids[3, ..., 1] == 3.0) and np.all(grids[..., 0] == 0)


# ---- padding and chunks ---------------------------------------------------------------------------------------------------------------
def test_pad_to_valid_T(host):
    assert [host.pad_to_valid_T(t) for t in (1, 3, 9, 224, 225, 226)] == [9, 9, 9, 225, 225, 237]
    for t in range(1, 500):
        p = host.pad_to_valid_T(t)
        assert p >= t and (p + 3) % 4 == 0 and ((p + 3) // 4) % 3 == 0 and p - 12 < t
    with pytest.raises(ValueError):
        host.pad_to_valid_T(0)


def test_chunk_schedule(host):
    assert host.chunk_schedule(1) == [(True, True, 0, 1, (0, 1))]
    assert host.chunk_schedule(6) == [(True, True, 0, 6, (0, 6))]
    assert host.chunk_schedule(225) == [(True, False, 0, 225, (0, 222)), (False, True, 219, 6, (222, 225))]
    assert host.chunk_schedule(226) == [(True, False, 0, 225, (0, 222)), (False, True, 219, 7, (222, 226))]
    assert host.chunk_schedule(450) == [(True, False, 0, 225, (0, 222)), (False, False, 219, 225, (222, 441)), (False, True, 438, 12, (441, 450))]
    from metric_depth_video_toolbox_amd import infill_clip
    for n in (1, 24, 25, 26, 44, 45, 100):
        assert host.chunk_schedule(n, 25) == infill_clip.chunk_schedule(n)
    for n, chunk in ((29, 10), (450, 225), (17, 7)):                 # every frame is written exactly once, in order
        written = [t for *_, (a, b) in host.chunk_schedule(n, chunk) for t in range(a, b)]
        assert written == list(range(n))
    with pytest.raises(ValueError):
        host.chunk_schedule(10, 6)


# ---- the header and its binding -------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_by_both_libraries_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(HEADER)
    assert sorted(decls) == sorted(_lib.INSPATIO_SYMBOLS) == NAMES
    L, T = _lib.load(), ctypes.CDLL(_lib.lib_path("tuning"))
    main_header = open(os.path.join(REPO, "include", "mdvt.h")).read()
    own_unit = open(os.path.join(CSRC, "mdvt_api_inspatio.hip")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    for name, args in decls.items():
        assert hasattr(L, name) and hasattr(T, name), name
        assert name not in _lib.SYMBOLS and name not in main_header
        assert re.search(r"^int " + name + r"\(", own_unit, flags=re.M)
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in args.split(",")]
        assert getattr(L, name).argtypes == want and getattr(L, name).restype is ctypes.c_int, name
        for a in args.split(","):                                   # pitches and strides are 64-bit
            if re.search(r"(pitch|stride)$", a.strip()):
                assert a.split()[0] == "size_t", a
    for name in ("mdvt_masked_shift_grid", "mdvt_flow_warp", "mdvt_inspatio_prepare_eye", "mdvt_inspatio_model_frames", "mdvt_inspatio_composite_eye"):
        assert decls[name].startswith("mdvt_ctx* ctx,") and decls[name].endswith("void* stream") and name not in _lib.NO_STREAM
    assert L.mdvt_version() == 15                                   # include/mdvt.h is unchanged
    text = open(HEADER).read()
    for cited in ("iwi:76-115, 154-168", "RESTATED, NOT OBSERVED", "DECREE", "0.3", "1000 * 2^-23"):
        assert cited in text, f"the header cites {cited}"


def test_a_null_context_is_refused_and_the_path_query_needs_no_device():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert L.mdvt_masked_shift_grid(None, 16, 16, 1, None, 48, 0, None, 48, 0, None, 16, 0, 0, None, None, None, None) == -1
    assert L.mdvt_flow_warp(None, 16, 16, 1, None, None, None, 48, 0, None, 48, 0, None) == -1
    for (W, H), want in (((90, 46), 1), ((41, 33), 1), ((256, 256), 1), ((257, 256), 2), ((960, 1080), 2), ((4096, 4096), 2), ((8, 8), 1),
                         ((7, 8), 0), ((8, 7), 0), ((4097, 64), 0), ((64, 4097), 0)):
        assert L.mdvt_masked_shift_path(W, H) == want == ir.path_of(W, H), (W, H)


def test_the_package_module_imports_no_torch_and_takes_no_address(host):
    src = open(host.__file__).read()
    assert "data_ptr" not in src and "import torch" not in src and "from torch" not in src
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); import metric_depth_video_toolbox_amd.inspatio_world as s; "
                        "s.pad_to_valid_T(5); s.chunk_schedule(9); print('torch' in sys.modules)", REPO], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stderr[-2000:]


# ---- the tool's refusals and texts ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("inspatio_world_infill_tool", os.path.join(REPO, "tools", "inspatio_world_infill.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tool_refuses_before_anything_is_opened(tool, tmp_path):
    names = {k: str(tmp_path / (k + ".mkv")) for k in ("org", "sbs", "mask")}
    for p in names.values():
        open(p, "wb").close()
    base = ["--color_video", names["org"], "--sbs_color_video", names["sbs"], "--sbs_mask_video", names["mask"]]
    with pytest.raises(NotImplementedError, match="--lower_mask_dilation is left out: it repaints the render"):
        tool.main(base + ["--lower_mask_dilation", "2"])
    with pytest.raises(SystemExit, match="--max_frames 0"):
        tool.main(base + ["--max_frames", "0"])
    with pytest.raises(SystemExit, match="input color_video does not exist"):
        tool.main(["--color_video", str(tmp_path / "none.mkv")] + base[2:])
    with pytest.raises(ValueError, match="--chunk must be above the 6 frames kept"):
        tool.main(base + ["--chunk", "6"])
    # the default wrapper imports its model lazily and fails with one line without it
    with pytest.raises(SystemExit) as e:
        tool.main(base)
    assert "the inspatio_world generator needs the inspatio-world checkout" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit, match="--generator must be 'inspatio_world' or 'pkg.module:callable'"):
        tool.main(base + ["--generator", "nothing"])
    # lists: all three, of equal length
    lst = str(tmp_path / "l.txt")
    open(lst, "w").write(names["sbs"] + "\n")
    with pytest.raises(ValueError, match="If --sbs_color_video is a .txt file, then --sbs_mask_video and --color_video must also be .txt files"):
        tool.main(["--color_video", names["org"], "--sbs_color_video", lst, "--sbs_mask_video", names["mask"]])
    two = str(tmp_path / "two.txt")
    open(two, "w").write(names["mask"] + "\n" + names["mask"] + "\n")
    with pytest.raises(ValueError, match="List length mismatch"):
        tool.main(["--color_video", lst, "--sbs_color_video", lst, "--sbs_mask_video", two])
    assert sorted(os.listdir(tmp_path)) == ["l.txt", "mask.mkv", "org.mkv", "sbs.mkv", "two.txt"]
    doc = tool.__doc__
    for said in ("generate(source, render, mask, fps, text_prompt) -> frames", "UNTESTED", "NOT WIRED INTO THE DRIVER", "follow-up"):
        assert said in doc, said
    assert "import torch" not in open(tool.__file__).read().split("def _padded")[0], "torch is imported inside the functions"
