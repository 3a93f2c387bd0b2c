"""The per-frame depth engines' and PromptDA's steps, host side -- no GPU: the new header and its binding, the parsers, the file names
with their tmp -> rename step, the --max_frames count, the two refused scripts, closest_higher_multiple, the three x-fov variants and
the NumPy restatement of the focal estimate (tests/depth_engines_ref.py), all held to tests/golden/depth_engines.npz, which
tests/golden/gen_depth_engines_golden.py wrote from the reference's own functions."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import depth_engines_ref as er
import footprint as fp
import metric_align_ref as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdvt_depth_engines.h")
GOLDEN = os.path.join(REPO, "tests", "golden", "depth_engines.npz")
FOCAL_CASES = ("noisy96", "clean40x30", "special7x3", "empty7x3")
F = np.float32


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def host():
    from metric_depth_video_toolbox_amd import depth_engines
    return depth_engines


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the header and its binding -----------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_by_both_libraries_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(HEADER)
    assert sorted(decls) == sorted(_lib.DEPTH_ENGINE_SYMBOLS) == ["mdvt_depth_prompt", "mdvt_focal_from_points", "mdvt_model_frames"]
    L, T = _lib.load(), ctypes.CDLL(_lib.lib_path("tuning"))
    main_header = open(os.path.join(REPO, "include", "mdvt.h")).read()
    api_unit = open(os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc", "mdvt_api.hip")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    for name, args in decls.items():
        assert hasattr(L, name) and hasattr(T, name), name
        assert name not in _lib.SYMBOLS and name not in _lib.DEPTH_SINK_SYMBOLS
        assert name not in main_header and not re.search(r"^int " + name + r"\(", api_unit, flags=re.M)
        # the bound prototype is the declaration's, parameter by parameter
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in args.split(",")]
        assert getattr(L, name).argtypes == want and getattr(L, name).restype is ctypes.c_int, name
        assert args.startswith("mdvt_ctx* ctx,") and args.endswith("void* stream")
    assert L.mdvt_version() == 15                                   # include/mdvt.h is unchanged
    # the existing tuples keep their contents
    assert _lib.DEPTH_SINK_SYMBOLS == ("mdvt_depth_video_codes",) and not set(_lib.DEPTH_ENGINE_SYMBOLS) & set(_lib.SYMBOLS)


def test_a_null_context_is_refused_without_a_device():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert L.mdvt_model_frames(None, 4, 4, 1, None, 12, 48, 0, 4, 4, 0, None, 4, 16, 48, None) == -1
    assert L.mdvt_depth_prompt(None, 4, 4, 1, None, 12, 48, 0, 100.0, 4, 4, None, 16, 64, None) == -1
    assert L.mdvt_focal_from_points(None, 4, 4, 1, None, 0, 16, 64, 192, None, None, None) == -1


# ---- parsers, names, counts ---------------------------------------------------------------------------------------------------------
def test_the_parsers_defaults_are_the_references(host):
    a = host.build_engine_parser().parse_args(["--engine", "unik3d", "--color_video", "x.mkv"])
    assert (a.max_frames, a.target_fps, a.max_depth, a.xfov, a.yfov) == (-1, -1, 100, None, None)
    assert (a.generator, a.batch, a.video_decoder, a.video_encoder) == (None, 8, "host", "host")
    a = host.build_engine_parser().parse_args(["--engine", "moge", "--color_video", "x", "--max_depth", "20", "--xfov", "55.5", "--target_fps", "12"])
    assert isinstance(a.max_depth, int) and a.max_depth == 20 and a.xfov == 55.5 and a.target_fps == 12
    host.check_engine_flags(a)
    with pytest.raises(SystemExit):
        host.build_engine_parser().parse_args(["--color_video", "x.mkv"])            # --engine is required
    p = host.build_promptda_parser().parse_args(["--color_video", "x.mkv", "--depth_video", "d.mkv"])
    assert (p.max_frames, p.max_depth, p.generator, p.batch, p.video_decoder, p.video_encoder) == (-1, 100, "promptda", 4, "host", "host")
    with pytest.raises(SystemExit):
        host.build_promptda_parser().parse_args(["--color_video", "x.mkv"])          # --depth_video is required
    assert (host.PROMPT_W, host.PROMPT_H) == (256, 192)


def test_depthpro_takes_no_field_of_view_and_a_batch_is_at_least_one(host):
    a = host.build_engine_parser().parse_args(["--engine", "depthpro", "--color_video", "x.mkv", "--xfov", "60"])
    with pytest.raises(ValueError, match="depthpro_video.py"):
        host.check_engine_flags(a)
    a = host.build_engine_parser().parse_args(["--engine", "moge", "--color_video", "x.mkv", "--batch", "0"])
    with pytest.raises(ValueError, match="--batch"):
        host.check_engine_flags(a)
    with pytest.raises(ValueError, match="--engine"):
        host.check_engine("depthcrafter")


@pytest.mark.parametrize("engine,why", [("unidepth", r"unidepth_video\.py:80.*fps"), ("videoanythingmetric", r"read_video_frames")])
def test_the_two_scripts_left_out_are_refused_before_a_file_is_opened(host, tmp_path, engine, why):
    tool = _tool("depth_engine_video")
    missing = str(tmp_path / "no_such_clip.mkv")                    # were a file opened, this would fail first, with another error
    args = host.build_engine_parser().parse_args(["--engine", engine, "--color_video", missing, "--generator", "no.such.module:fn"])
    with pytest.raises(NotImplementedError, match=why):
        tool.run(args)
    assert os.listdir(tmp_path) == []


def test_the_default_generators_fail_with_one_line_where_their_packages_are_missing(host, monkeypatch):
    import sys
    for engine, packages in (("unik3d", ("unik3d", "unik3d.models")), ("moge", ("moge", "moge.model")), ("depthpro", ("depth_pro",)),
                             ("promptda", ("promptda", "promptda.promptda"))):
        for p in packages:
            monkeypatch.setitem(sys.modules, p, None)               # (an import of it raises ImportError, installed or not)
        for spec in (None, engine):
            with pytest.raises(RuntimeError, match=packages[0]) as e:
                host.load_generator(spec, engine)
            assert "\n" not in str(e.value)
    with pytest.raises(ValueError):
        host.load_generator("not_a_spec", "moge")
    with pytest.raises(ValueError):
        host.load_generator("da3", "moge")
    assert host.load_generator("json:dumps", "moge") is json.dumps  # pkg.module:callable, through video_da3.load_generator


def test_file_names_and_the_tmp_rename_step(host, tmp_path):
    assert host.engine_output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_xfovs.json")
    assert host.engine_output_paths("x.npy", video=False) == ("x.npy_tmp_depth.npy", "x.npy_depth.npy", "x.npy_depth.npy_xfovs.json")
    assert host.promptda_output_paths("d.mkv") == ("d.mkv_tmp_upscaled.mkv", "d.mkv_upscaled.mkv")
    assert host.promptda_output_paths("d.npy", video=False) == ("d.npy_tmp_upscaled.npy", "d.npy_upscaled.npy")
    lst = tmp_path / "clips.txt"
    lst.write_text("# a list\n\n a.mkv \nb.mkv\n")
    assert host.clips_from_argument(str(lst)) == ["a.mkv", "b.mkv"] and host.clips_from_argument("a.mkv") == ["a.mkv"]
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    for tmp, final in (host.engine_output_paths(str(tmp_path / "c.npy"), video=False)[:2], host.promptda_output_paths(str(tmp_path / "d.npy"), video=False)):
        with ClipOutput(tmp, final, 2, (2, 3, 3)) as out:
            assert os.path.exists(tmp) and not os.path.exists(final)
            out.arr[...] = 7
        assert os.path.exists(final) and not os.path.exists(tmp) and np.load(final).shape == (2, 2, 3, 3)
        os.remove(final)
        with pytest.raises(KeyError):
            with ClipOutput(tmp, final, 2, (2, 3, 3)):
                raise KeyError("the batch loop failed")
        assert not os.path.exists(tmp) and not os.path.exists(final)
    xf = str(tmp_path / "x.json")
    host.write_xfovs(xf, [np.float32(45.5), 60.0])
    assert json.load(open(xf)) == [45.5, 60.0]


def test_max_frames_writes_exactly_that_many(host):
    def reference_loop(n_in_file, max_frames):                       # u3d:154-163 as written
        frame_n, written = 0, 0
        for _ in range(n_in_file):
            frame_n += 1
            if max_frames < frame_n and max_frames != -1:
                break
            written += 1
        return written
    for n in (1, 5, 12):
        for m in (-1, 0, 1, 4, 5, 6, 12, 13, 100):
            assert host.frames_to_write(n, m) == reference_loop(n, m), (n, m)
    assert host.frames_to_write(12, 5) == 5 and host.frames_to_write(12, -1) == 12


def test_closest_higher_multiple(host, golden):
    for x, want in zip(golden["chm_in"], golden["chm_out"]):
        assert host.closest_higher_multiple(int(x)) == er.closest_higher_multiple(int(x)) == int(want)
    assert host.closest_higher_multiple(1080) == 1092 and host.closest_higher_multiple(1920) == 1932 and host.closest_higher_multiple(28) == 28


# ---- the x-fov variants -------------------------------------------------------------------------------------------------------------
def test_the_three_x_fov_variants_equal_the_references(host, golden):
    for (fx, fy, W, H), want in zip(golden["fov_unik3d_in"], golden["fov_unik3d_out"]):
        got = host.xfov_unik3d(F(fx), F(fy), int(W), int(H))
        assert got == want == er.xfov_f64(F(fx), int(W)) and isinstance(got, float)
    assert golden["fov_unik3d_out"][-1] == 180.0                    # a focal estimate of 0 (nothing selected)
    for K, want in zip(golden["fov_moge_in"], golden["fov_moge_out"]):
        got = host.xfov_moge(K)
        assert got == want == er.xfov_f32(K)
        assert F(got) == got                                        # float32 arithmetic: the value is a float32
    assert any(F(v) != v for v in golden["fov_unik3d_out"])         # ... which the float64 variants' values are not
    for (f, W, H), want in zip(golden["fov_depthpro_in"], golden["fov_depthpro_out"]):
        assert host.xfov_depthpro(F(f), int(W), int(H)) == want == er.xfov_f64(float(f), int(W))
    cam = host.requested_camera(60.0, None, 64, 36)
    assert cam.dtype == np.float32 and host.requested_camera(None, None, 64, 36) is None
    assert abs(host.xfov_moge(cam) - 60.0) < 1e-4


# ---- the focal estimate's restatement against torch's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FOCAL_CASES)
def test_values_and_selections_equal_torchs_bit_for_bit(golden, case):
    points = er.channel_last(golden[f"focal_{case}_points"])
    assert points.shape[0] == 1
    ex, ey, mx, my = er.focal_values(points[0])
    assert np.array_equal(mx, golden[f"focal_{case}_mx"]) and np.array_equal(my, golden[f"focal_{case}_my"])
    # the reference's arrays hold 0 where nothing is selected (its torch.where); selected values bit for bit, NaN for NaN
    for e, m, want in ((ex, mx, golden[f"focal_{case}_ex"]), (ey, my, golden[f"focal_{case}_ey"])):
        assert mr.same_bits(np.where(m, e, F(0)), want).size == 0
        assert not np.any(want[~m])


@pytest.mark.parametrize("case", FOCAL_CASES)
def test_means_are_within_the_summation_bound_of_torchs(golden, case):
    """The order of the sum is this project's (the header's decree); torch's is another.  Two float32 sums of the same n values in
    any two orders each err by at most (n - 1) 2^-24 sum|e| (to first order; Higham, Accuracy and Stability, eq. 4.4), so they
    differ by at most twice that, and the means by 2 (n - 1) 2^-24 sum|e| / n: the bound the header decrees."""
    points = er.channel_last(golden[f"focal_{case}_points"])
    ex, ey, mx, my = er.focal_values(points[0])
    ours, counts = er.focal(points)
    assert counts[0].tolist() == [int(mx.sum()), int(my.sum())]
    for k, (e, m) in enumerate(((ex, mx), (ey, my))):
        theirs, n = golden[f"focal_{case}_f"][k], int(m.sum())
        if n == 0:
            assert ours[0, k] == 0.0 and theirs == 0.0 and np.signbit(ours[0, k]) == np.signbit(theirs)
            continue
        mag = np.abs(e[m].astype(np.float64)).sum()
        if not np.isfinite(mag):                                     # an infinity or a NaN among the selected: IEEE decides, in any order
            assert (np.isnan(ours[0, k]) and np.isnan(theirs)) or ours[0, k] == theirs
            continue
        bound = 2 * (n - 1) * 2.0 ** -24 * mag / n
        print(f"{case} axis {k}: n = {n}, ours {ours[0, k]!r}, torch {theirs!r}, |difference| {abs(float(ours[0, k]) - float(theirs)):.3e}, bound {bound:.3e}")
        assert abs(float(ours[0, k]) - float(theirs)) <= bound


def test_np_sum_is_the_order_spelled_out_and_the_inputs_tell_the_orders_apart(golden):
    """depth_engines_ref.focal sums with np.sum; metric_align_ref.sum_chunked spells the same order out.  With
    metric_align_ref.orders_told_apart's method: some list of the golden inputs sums differently left to right, and some differently
    in float64 rounded once, so a device sum in either of those orders would fail the GPU tests."""
    ltr = f64 = False
    for case in FOCAL_CASES:
        points = er.channel_last(golden[f"focal_{case}_points"])
        ex, ey, mx, my = er.focal_values(points[0])
        assert mr.same_bits(er.focal(points)[0], er.focal(points, total=mr.sum_chunked)[0]).size == 0, case
        for e, m in ((ex, mx), (ey, my)):
            sel = np.ascontiguousarray(e[m])
            if sel.size == 0 or not np.isfinite(sel).all():
                continue
            ours = np.sum(sel)
            ltr |= ours.tobytes() != mr.sum_left_to_right(sel).tobytes()
            f64 |= ours.tobytes() != mr.sum_f64_rounded(sel).tobytes()
    assert ltr and f64
    assert int(golden["focal_noisy96_my"].sum()) > 8192 > int(golden["focal_noisy96_mx"].sum())       # both sides of a chunk edge


def test_the_restated_layouts_and_formats_agree():
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 5, 13, 3), dtype=np.uint8)
    u8 = er.model_frames(frames)
    assert u8.shape == (2, 3, 5, 13) and np.array_equal(u8, frames.transpose(0, 3, 1, 2))
    assert np.array_equal(er.model_frames(frames[..., ::-1], bgr=True), u8)
    f = er.model_frames(frames, as_float=True)
    assert f.dtype == np.float32 and np.array_equal(f, u8.astype(F) / F(255))
    v = np.arange(256, dtype=np.uint8)
    assert np.any(v.astype(F) / F(255) != v.astype(F) * F(1.0 / 255.0))                # it is not v * (1 / 255)
    assert er.model_frames(frames, (28, 14)).shape == (2, 3, 14, 28)
    codes = rng.integers(0, 256, (1, 6, 8, 3), dtype=np.uint8)
    d = er.depth_prompt(codes, 100, (8, 6))
    assert np.array_equal(d[0], er.decode(codes[0], 100)) and np.array_equal(er.depth_prompt(codes[..., ::-1], 100, (8, 6), bgr=True), d)
    pts = rng.normal(size=(2, 3, 7, 3)).astype(F)                   # [N, H, W, 3] with H = 3: the last dimension decides
    a, na = er.focal(pts)
    b, nb = er.focal(np.ascontiguousarray(pts.transpose(0, 3, 1, 2)))               # [N, 3, 3, 7]
    assert a.shape == (2, 2) and np.array_equal(na, nb) and mr.same_bits(a, b).size == 0
