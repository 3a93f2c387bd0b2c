"""The MegaSAM camera-tracking step without a GPU: tests/megasam_ref.py, the NumPy restatement the device is held to bit for bit, against
the exact box mean (the area resize), torch's CPU kernels (nearest-exact exactly, the mask's bilinear within the MVSAnywhere row's
bound B) and the library's own area-table builder in a program of its own; the host logic of
metric_depth_video_toolbox_amd/sam_track.py against hand-written values and torch's float32; the header and its binding; the
refusals, which write nothing."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import footprint as fp
import megasam_ref as gr
import mvsa_ref as mv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdvt_megasam.h")
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")
NAMES = ["mdvt_area_model_frames", "mdvt_megasam_vector_path", "mdvt_tracker_depth", "mdvt_tracker_mask", "mdvt_tracker_outputs"]
F = np.float32


@pytest.fixture(scope="module")
def host():
    from metric_depth_video_toolbox_amd import sam_track
    return sam_track


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("sam_track_video_tool", os.path.join(REPO, "tools", "sam_track_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- (a): the area restatement and the exact box mean ---------------------------------------------------------------------------------
# (in_w, in_h) -> (mid_w, mid_h)
AREA_PAIRS = [((29, 37), (9, 11)), ((13, 21), (8, 13)), ((33, 59), (10, 18)), ((16, 24), (5, 7))]


@pytest.mark.parametrize("pair", AREA_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_area_restatement_lies_within_half_a_step_of_the_exact_box_mean(pair):
    """The bound 0.501: the rounding to a byte costs at most 0.5; float32 weights and sums carry at most (taps + 2) * 2^-24 relative
    error on values <= 255, with at most 8 + 8 taps 255 * 18 * 2^-24 = 2.7e-4 < 1e-3."""
    (W, H), (w, h) = pair
    worst = 0.0
    for k, kind in enumerate(("noise", "extremes")):
        rng = np.random.default_rng(2500 + 10 * AREA_PAIRS.index(pair) + k)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == "noise" else (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        got = gr.area_planes(img, (w, h))
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        worst = max(worst, float(np.abs(got.astype(np.float64) - gr.box_mean(img, (w, h))).max()))
    print(f"{pair}: max |restatement - exact box mean| = {worst:.6f}")
    assert worst <= 0.501
    for ssize, dsize in ((W, w), (H, h)):
        _, count, wts = gr.area_table(ssize, dsize)
        sums = wts.astype(np.float64).sum(axis=1)
        print(f"{ssize} -> {dsize}: taps {int(count.min())} .. {int(count.max())}, max |sum of weights - 1| = {float(np.abs(sums - 1).max()):.3e}")
        assert float(np.abs(sums - 1).max()) <= 1e-6


def test_area_restatement_refuses_integer_factors_and_enlargement_and_copies_equal_sizes():
    img = np.random.default_rng(2540).integers(0, 256, (12, 8, 3), dtype=np.uint8)
    for mid in ((4, 6), (4, 4), (2, 3), (8, 6)):                   # 2 x 2, 2 x 3, 4 x 4, 1 x 2: integer on both axes
        with pytest.raises(ValueError, match="integer factors"):
            gr.area_planes(img, mid)
    for mid in ((9, 12), (8, 13), (16, 24)):
        with pytest.raises(ValueError, match="enlargement"):
            gr.area_planes(img, mid)
    assert np.array_equal(gr.area_planes(img, (8, 12)), img)
    assert np.array_equal(gr.area_planes(img, (8, 12), (5, 7)), img[:7, :5])
    one_axis = gr.area_planes(img, (8, 5))                          # a pass alone leaves the other axis
    assert one_axis.shape == (5, 8, 3)
    assert np.array_equal(gr.area_model_frames(img[None], (5, 7), (4, 6))[0], gr.area_planes(img, (5, 7))[:6, :4].transpose(2, 0, 1))


# ---- (b): nearest-exact ---------------------------------------------------------------------------------------------------------------
NEX_PAIRS = [((1920, 1080), (591, 332)), ((591, 332), (1920, 1080)), ((73, 41), (1920, 1080)), ((96, 54), (72, 40)), ((37, 29), (11, 9)),
             ((11, 9), (37, 29)), ((1280, 720), (591, 332)), ((3840, 2160), (591, 332)), ((101, 37), (37, 101)), ((5, 7), (5, 7))]


@pytest.mark.parametrize("pair", NEX_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_nearest_exact_restatement_equals_torch(pair):
    import torch
    import torch.nn.functional as TF
    (W, H), (w, h) = pair
    ramp = (np.arange(H, dtype=np.float64)[:, None] * 4096 + np.arange(W)[None, :]).astype(F)      # every value names its source pixel
    want = TF.interpolate(torch.from_numpy(ramp)[None, None], (h, w), mode="nearest-exact").squeeze().numpy()
    assert np.array_equal(gr.nex_planes(ramp, (w, h)), want.reshape(h, w))


# ---- (c): the depth and the mask ------------------------------------------------------------------------------------------------------
def test_tracker_depth_is_the_references_lines():
    import torch
    import torch.nn.functional as TF
    rng = np.random.default_rng(2560)
    rgb = rng.integers(0, 256, (2, 29, 37, 3), dtype=np.uint8)
    for max_depth in (100, 20):
        for k in range(2):
            depth = np.zeros((29, 37), dtype=np.uint32)             # stv:127-131
            unit = depth.view(np.uint8).reshape((29, 37, 4))
            unit[..., 3] = rgb[k, ..., 0].astype(np.uint32)
            unit[..., 2] = rgb[k, ..., 2]
            d = depth.astype(np.float32) / ((255 ** 4) / max_depth)
            assert d.dtype == np.float32
            want = TF.interpolate(torch.as_tensor(d)[None, None], (9, 11), mode="nearest-exact").squeeze()[:8, :8].numpy()
            got = gr.tracker_depth(rgb[k:k + 1], max_depth, (11, 9), (8, 8))[0]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("pair", [((37, 29), (11, 9)), ((96, 54), (72, 40)), ((1920, 1080), (591, 332))], ids=lambda p: f"{p[0][0]}x{p[0][1]}")
def test_tracker_mask_lies_within_the_bilinear_bound_of_torch(pair):
    import torch
    import torch.nn.functional as TF
    import convergence_ref as cr
    (W, H), (w, h) = pair
    rgb = np.random.default_rng(2570 + W).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    m = torch.as_tensor(255 - cr.gray_of(rgb[0])).float() / 255.0                               # stv:158
    want = TF.interpolate(m[None, None], (h, w), mode="bilinear").squeeze().numpy()[:h - h % 8, :w - w % 8]
    got = gr.tracker_mask(rgb, (w, h), (w - w % 8, h - h % 8))[0]
    B = mv.bilinear_bound(W, H)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{pair}: max |restatement - torch| = {worst:.3e}, B = {B:.3e}")
    assert got.shape == want.shape and worst <= B


def test_tracker_outputs_restatement_on_hand_made_values():
    p = np.array([[[-1.0, 0.0, 0.25, 0.5], [1.0, 2.0, np.nan, np.inf]]], F)
    grey = gr.tracker_outputs(p, 1, 1.0, (4, 2))
    assert grey[0, :, :, 0].tolist() == [[0, 0, 63, 127], [255, 255, 0, 255]] and np.array_equal(grey[..., 0], grey[..., 2])
    codes = gr.tracker_outputs(p, 0, 100.0, (4, 2))
    assert codes[0, 0, 0].tolist() == [0, 0, 0] and codes[0, 1, 2].tolist() == [0, 0, 0]       # below 0 and NaN: code 0
    with pytest.raises(ValueError, match="2 x reduction"):
        gr.tracker_outputs(np.zeros((1, 4, 8), F), 1, 1.0, (4, 2))


# ---- (d): the host logic --------------------------------------------------------------------------------------------------------------
def test_model_size_on_the_usual_sizes(host):
    for h0, w0 in ((1080, 1920), (2160, 3840), (720, 1280), (540, 960)):
        assert host.model_size(h0, w0) == (332, 591, 328, 584) == gr.model_size(h0, w0)
    assert host.model_size(54, 96) == (332, 591, 328, 584)          # 16:9 at any size: the tracker's size does not depend on the video's
    assert host.model_size(480, 640) == (384, 512, 384, 512)
    assert host.model_size(512, 512) == (443, 443, 440, 440)


def test_scaled_intrinsics_equal_torchs_float32(host):
    import torch
    for (w0, h0), xfov, yfov in (((1920, 1080), 60.0, None), ((1280, 720), None, 41.5), ((960, 540), 72.3, 44.0), ((96, 54), 55.0, None)):
        cam_matrix = host.camera_matrix(xfov, yfov, w0, h0)
        assert cam_matrix.dtype == np.float32
        h1, w1, _, _ = host.model_size(h0, w0)
        t = torch.as_tensor([cam_matrix[0, 0], cam_matrix[1, 1], cam_matrix[0, 2], cam_matrix[1, 2]])      # stv:138-140
        t[0::2] *= w1 / w0
        t[1::2] *= h1 / h0
        got = host.scaled_intrinsics(cam_matrix, h0, w0, h1, w1)
        assert t.dtype == torch.float32 and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), t.numpy().view(np.uint32))


def test_frame_plan_is_the_issues_table(host):
    N = 12
    assert host.frame_plan(N, N, None, -1) == (N - 1, None)          # equal lengths: the colour read behind the last frame ends the loop
    assert host.frame_plan(N, N, N, -1) == (N - 1, None)
    assert host.frame_plan(N, N + 1, None, -1) == (N, N - 1)          # a longer colour video: the last frame goes through track_final
    assert host.frame_plan(N, N + 1, N + 1, -1) == (N, N - 1)
    assert host.frame_plan(N, N + 1, N, -1) == (N - 1, None)          # ... unless the mask video ends with the depth video
    for M in (0, 1, 3, N - 3):
        assert host.frame_plan(N, N, None, M) == (M + 2, M + 1)       # --max_frames M with N >= M + 3
    for M in (N - 2, N - 1, N, 50):
        assert host.frame_plan(N, N, None, M) == (N - 1, None)        # N < M + 3, equal lengths
    assert host.frame_plan(1, 1, None, -1) == (0, None)
    for short in ((N, N - 1, None), (N, N, N - 1)):
        with pytest.raises(ValueError, match="crashes on the missing frame"):
            host.frame_plan(*short, -1)
    # the loop, followed read by read, against the closed form of the restatement
    for n in range(1, 9):
        for extra_c in (0, 1, 3):
            for n_mask in (None, n, n + 2):
                for M in (-1, 0, 1, 2, 3, 5, 7, 9):
                    assert host.frame_plan(n, n + extra_c, n_mask, M) == gr.frame_plan(n, n + extra_c, n_mask, M), (n, extra_c, n_mask, M)


def test_poses_to_transformations(host):
    rng = np.random.default_rng(2580)
    q = rng.standard_normal((6, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    traj = np.concatenate([rng.standard_normal((6, 3)) * 3, q], axis=1)
    T = host.poses_to_transformations(traj)
    assert T.shape == (7, 4, 4) and T.dtype == np.float64 and np.array_equal(T[0], np.eye(4))     # the identity row (stv:240)
    for p, inv in zip(traj, T[1:]):
        assert float(np.abs(gr.pose_matrix(p) @ inv - np.eye(4)).max()) <= 1e-12
    hand = host.poses_to_transformations([[1.0, -2.0, 0.5, 0, 0, 0, 1],                            # a pure translation
                                          [1.0, 0.0, 0.0, 0, np.sqrt(0.5), 0, np.sqrt(0.5)]])       # a 90 degree turn about y, then x + 1
    assert np.array_equal(hand[1], [[1, 0, 0, -1], [0, 1, 0, 2], [0, 0, 1, -0.5], [0, 0, 0, 1]])
    # R = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]; R^T = [[0, 0, -1], [0, 1, 0], [1, 0, 0]]; -R^T t = (0, 0, -1)
    assert np.allclose(hand[2], [[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, -1], [0, 0, 0, 1]], atol=1e-15)
    with pytest.raises(ValueError, match=r"\[t, 7\]"):
        host.poses_to_transformations(np.zeros((3, 6)))


def test_estimated_fov_is_the_references_lines(host):
    fovx, fovy = host.estimated_fov(np.array([63.9, 63.9, 36.5, 20.5], F))
    k = np.array([63.9, 63.9, 36.5, 20.5], F) * 8
    assert fovx == np.rad2deg(2 * np.arctan2(float(k[2]) * 2, 2 * float(k[0]))) and fovy == np.rad2deg(2 * np.arctan2(float(k[3]) * 2, 2 * float(k[1])))


def test_the_parsers_defaults_and_the_names_are_the_references(host):
    a = host.build_parser().parse_args(["--color_video", "x.mkv", "--depth_video", "x.mkv_depth.mkv"])
    assert (a.mask_video, a.max_frames, a.max_depth, a.xfov, a.yfov, a.optimize_intrinsic) == (None, -1, 100, None, None, False)
    assert (a.batch, a.video_decoder, a.video_encoder, a.generator) == (8, "host", "host", "megasam")
    paths = host.output_paths("x.mkv_depth.mkv")
    assert paths["json"][1] == "x.mkv_depth.mkv_transformations.json"                          # stv:46
    assert paths["depth"][1] == "x.mkv_depth.mkv_megasam.mkv" and paths["motion"][1] == "x.mkv_depth.mkv_megasam_motion.mkv"
    assert all(tmp != final and "_tmp_" in tmp for tmp, final in paths.values())
    assert host.output_paths("d.npy", video=False)["depth"][1] == "d.npy_megasam.npy"
    with pytest.raises(ValueError, match="'megasam' or 'pkg.module:callable'"):
        host.load_generator("nonsense")


def test_refusals_name_their_reason_and_write_nothing(host, tool, tmp_path):
    color, depth, short = tmp_path / "c.npy", tmp_path / "d.npy", tmp_path / "s.npy"
    np.save(color, np.zeros((4, 54, 96, 3), np.uint8))
    np.save(depth, np.zeros((4, 54, 96, 3), np.uint8))
    np.save(short, np.zeros((3, 54, 96, 3), np.uint8))
    np.save(tmp_path / "other.npy", np.zeros((4, 27, 48, 3), np.uint8))
    before = sorted(os.listdir(tmp_path))

    def make_tracker(size):
        raise AssertionError("the tracker is not reached")
    base = ["--color_video", str(color), "--depth_video", str(depth)]
    with pytest.raises(ValueError, match="Either --xfov or --yfov is required"):
        tool.run(host.build_parser().parse_args(base), make_tracker)
    with pytest.raises(ValueError, match="must be at least 1"):
        tool.run(host.build_parser().parse_args(base + ["--xfov", "60", "--batch", "0"]), make_tracker)
    with pytest.raises(Exception, match="input mask_video does not exist"):
        tool.run(host.build_parser().parse_args(base + ["--xfov", "60", "--mask_video", str(tmp_path / "none.npy")]), make_tracker)
    with pytest.raises(ValueError, match="the color video has 3 frames, the depth video 4"):
        tool.run(host.build_parser().parse_args(["--color_video", str(short), "--depth_video", str(depth), "--xfov", "60"]), make_tracker)
    with pytest.raises(ValueError, match="the mask video has 3 frames"):
        tool.run(host.build_parser().parse_args(base + ["--xfov", "60", "--mask_video", str(short)]), make_tracker)
    with pytest.raises(ValueError, match="must have one size"):
        tool.run(host.build_parser().parse_args(["--color_video", str(tmp_path / "other.npy"), "--depth_video", str(depth), "--xfov", "60"]), make_tracker)
    assert sorted(os.listdir(tmp_path)) == before


# ---- (e): the library's table builder, in a program of its own -------------------------------------------------------------------------
TABLE_PAIRS = [(29, 9), (37, 11), (13, 8), (21, 13), (33, 10), (59, 18), (16, 5), (24, 7), (1920, 591), (1080, 332), (3840, 591), (7, 7),
               (1, 1), (16384, 3), (8, 4), (9, 12), (16385, 4), (0, 4)]


def _build_table_program(sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        return None, "no g++"
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="area_table_"), "area_table_host_asan" if sanitize else "area_table_host")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
           os.path.join(REPO, "tests", "area_table_host.cpp")]
    if sanitize:
        cmd[3:3] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and sanitize and any(t in r.stderr for t in ("cannot find -lasan", "cannot find -lubsan", "libasan.a", "libubsan.a", "unrecognized")):
        return None, r.stderr[-400:]
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_the_librarys_area_tables_equal_the_restatements(sanitize, tmp_path):
    exe, why = _build_table_program(sanitize)
    if exe is None:
        pytest.skip(why)
    res = str(tmp_path / "tables.bin")
    r = subprocess.run([exe, res] + [str(v) for p in TABLE_PAIRS for v in p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    words = np.fromfile(res, np.int32)
    at = 0
    for n_in, n_out in TABLE_PAIRS:
        ok, a, b, ktaps = (int(v) for v in words[at:at + 4])
        at += 4
        assert (a, b) == (n_in, n_out)
        if n_in < 1 or n_in > 16384 or n_out > n_in:
            assert ok == 0, (n_in, n_out)
            continue
        assert ok == 1, (n_in, n_out)
        first, count, w = gr.area_table(n_in, n_out)
        assert ktaps == w.shape[1]
        assert np.array_equal(words[at:at + n_out], first)
        assert np.array_equal(words[at + n_out:at + 2 * n_out], count)
        assert np.array_equal(words[at + 2 * n_out:at + 2 * n_out + n_out * ktaps].view(np.uint32), w.reshape(-1).view(np.uint32)), (n_in, n_out)
        assert int((first + count).max()) <= n_in and int(first.min()) >= 0 and int(count.min()) >= 1
        at += 2 * n_out + n_out * ktaps
    assert at == len(words)


# ---- (f): the header and its binding ----------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_by_both_libraries_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(HEADER)
    assert sorted(decls) == sorted(_lib.MEGASAM_SYMBOLS) == NAMES
    L, T = _lib.load(), ctypes.CDLL(_lib.lib_path("tuning"))
    main_header = open(os.path.join(REPO, "include", "mdvt.h")).read()
    api_unit = open(os.path.join(CSRC, "mdvt_api.hip")).read()
    own_unit = open(os.path.join(CSRC, "mdvt_api_megasam.hip")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    for name, args in decls.items():
        assert hasattr(L, name) and hasattr(T, name), name
        assert name not in _lib.SYMBOLS and name not in main_header
        assert not re.search(r"^int " + name + r"\(", api_unit, flags=re.M) and re.search(r"^int " + name + r"\(", own_unit, flags=re.M)
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in args.split(",")]
        assert getattr(L, name).argtypes == want and getattr(L, name).restype is ctypes.c_int, name
        if name == "mdvt_megasam_vector_path":                      # a pure function of a layout: no context, no stream
            continue
        assert args.startswith("mdvt_ctx* ctx,") and args.endswith("void* stream") and name not in _lib.NO_STREAM
        assert re.search(r"\bint bgr\b", args), name
        for a in args.split(","):                                   # pitches and strides are 64-bit
            if re.search(r"(pitch|stride)$", a.strip()):
                assert a.split()[0] == "size_t", a
    assert L.mdvt_version() == 15                                   # include/mdvt.h is unchanged
    text = open(HEADER).read()
    for cited in ("stv:124, 143-148", "stv:125-131, 150-154", "stv:156-165", "stv:222-234", "dfh:211-230", "RESTATED, NOT OBSERVED", "DECREE"):
        assert cited in text, f"the header cites {cited}"


def test_a_null_context_is_refused_and_the_path_query_needs_no_device():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert L.mdvt_area_model_frames(None, 8, 8, 1, None, 24, 192, 0, 5, 5, 4, 4, None, 4, 16, 48, None) == -1
    assert L.mdvt_tracker_depth(None, 8, 8, 1, None, 24, 192, 0, 100.0, 5, 5, 4, 4, None, 16, 64, None) == -1
    assert L.mdvt_tracker_mask(None, 8, 8, 1, None, 24, 192, 0, 5, 5, 4, 4, None, 16, 64, None) == -1
    assert L.mdvt_tracker_outputs(None, 0, 4, 4, 1, None, 16, 64, 100.0, 8, 8, None, 24, 192, 0, None) == -1
    assert L.mdvt_megasam_vector_path(6, 1, 4096, 32, 8) == 1       # one frame: its stride does not count
    assert L.mdvt_megasam_vector_path(6, 2, 4096, 32, 8) == 0
    assert L.mdvt_megasam_vector_path(5, 1, 4096, 32, 0) == 0       # 15 bytes: no whole 16-byte load in a row
    assert L.mdvt_megasam_vector_path(6, 1, 4097, 32, 0) == 0 and L.mdvt_megasam_vector_path(6, 1, 4096, 24, 0) == 0


def test_the_package_module_imports_no_torch_and_takes_no_address(host):
    src = open(host.__file__).read()
    assert "data_ptr" not in src and "UNTESTED" in src
    assert "import torch" not in src and "from torch" not in src
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); import metric_depth_video_toolbox_amd.sam_track as s; "
                        "s.frame_plan(5, 5, None, -1); s.poses_to_transformations([[0, 0, 0, 0, 0, 0, 1]]); print('torch' in sys.modules)", REPO],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stderr[-2000:]
