"""The MVSAnywhere step without a GPU: tests/mvsa_ref.py, the NumPy restatement the device is held to bit for bit, against torch's CPU
kernels -- the bilinear resize bit for bit where torch's bits are defined (exact scales, the plain kernel, several threads: a child
process) and within the derived bound B elsewhere, the nearest maps exactly, the median exactly; the host logic of
metric_depth_video_toolbox_amd/video_mvsa.py against hand-written values; the header and its binding; the refusals, which write
nothing."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import footprint as fp
import mvsa_ref as vr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdvt_mvsa.h")
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")
NAMES = ["mdvt_bilinear_model_frames", "mdvt_nearest_depth_codes", "mdvt_ratio_median"]
F = np.float32


@pytest.fixture(scope="module")
def host():
    from metric_depth_video_toolbox_amd import video_mvsa
    return video_mvsa


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("video_mvsa_tool", os.path.join(REPO, "tools", "video_mvsa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- (a): the bilinear restatement and torch's CPU kernel -------------------------------------------------------------------------------
# (in_w, in_h) -> (out_w, out_h) whose in / out is exactly representable on both axes
EXACT_PAIRS = [((1920, 1080), (1024, 576)), ((1280, 720), (1024, 576)), ((640, 480), (1024, 768)), ((30, 18), (16, 8)), ((15, 9), (8, 4))]
INEXACT_PAIRS = [((37, 53), (41, 64)), ((100, 100), (33, 77)), ((1920, 1080), (1022, 575))]

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.nn.functional as TF
import mvsa_ref as vr
torch.set_num_threads(8)
out = {"capability": torch.backends.cpu.get_cpu_capability(), "threads": torch.get_num_threads(), "pairs": []}
for k, ((W, H), (w, h)) in enumerate(json.loads(sys.argv[2])):
    rgb = np.random.default_rng(2300 + k).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    t = torch.from_numpy(rgb[0]).permute(2, 0, 1).float() / 255.0                      # video_mvsa.py:62
    want = TF.interpolate(t.unsqueeze(0), size=(h, w), mode="bilinear", align_corners=False).numpy()
    got = vr.bilinear_model_frames(rgb, (w, h))
    out["pairs"].append([int((got.view(np.uint32) != want.view(np.uint32)).sum()), int(got.size)])
print(json.dumps(out))
"""


def test_bilinear_restatement_is_torchs_plain_kernel_bit_for_bit_at_exact_scales():
    """A CPU-only child with ATEN_CPU_CAPABILITY=default and 8 threads: there torch's kernel is the unfused formula -- in two forms.
    torch's dispatch takes another kernel where out_w + out_h <= 128 (four weights fl(wy * wx), summed in order): held to the two-pass
    form alone, 160 of the 384 values of 30x18 -> 16x8 and 29 of the 96 of 15x9 -> 8x4 differ from F.interpolate by one unit in the last
    place, while the three large pairs are equal in every bit.  The restatement, and the library, follow torch's switch."""
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default", OMP_NUM_THREADS="8", MKL_NUM_THREADS="8")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "tests"), json.dumps(EXACT_PAIRS)], capture_output=True, text=True,
                       env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(got)
    if got["capability"].upper() != "DEFAULT":
        pytest.skip(f"THE CHILD REPORTS CPU CAPABILITY {got['capability']!r}, NOT 'DEFAULT': torch's plain bilinear kernel cannot be observed here")
    for pair, (differ, size) in zip(EXACT_PAIRS, got["pairs"]):
        assert size > 0 and differ == 0, f"{pair}: {differ} of {size} values differ from F.interpolate in their bits"


@pytest.mark.parametrize("pair", EXACT_PAIRS[3:] + INEXACT_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_bilinear_restatement_lies_within_the_derived_bound_of_torch(pair):
    """On this machine's own capability and thread count, exact and inexact scales alike."""
    import torch
    import torch.nn.functional as TF
    (W, H), (w, h) = pair
    rgb = np.random.default_rng(2310 + W).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    t = torch.from_numpy(rgb).permute(0, 3, 1, 2).float() / 255.0
    want = TF.interpolate(t, size=(h, w), mode="bilinear", align_corners=False).numpy()
    got = vr.bilinear_model_frames(rgb, (w, h))
    B = vr.bilinear_bound(W, H)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{pair}: max |restatement - torch| = {worst:.3e}, B = {B:.3e}")
    assert got.shape == want.shape == (2, 3, h, w) and worst <= B


def test_the_bound_is_the_stated_formula():
    assert vr.bilinear_bound(37, 53) == 2.0 ** -18 + 2.0 ** -18 + 2.0 ** -22            # 7.9e-6: a source index below 64 has units of 2^-18
    assert vr.bilinear_bound(1920, 1080) == 2.0 ** -13 + 2.0 ** -13 + 2.0 ** -22
    assert vr.bilinear_bound(64, 64) == 2.0 ** -18 + 2.0 ** -18 + 2.0 ** -22


def test_equal_sizes_give_the_division():
    rgb = np.random.default_rng(2320).integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    want = rgb.transpose(0, 3, 1, 2).astype(F) / F(255)
    assert np.array_equal(vr.bilinear_model_frames(rgb).view(np.uint32), want.view(np.uint32))


# ---- (b): the nearest maps ----------------------------------------------------------------------------------------------------------
# (in_w, in_h) -> (mid_w, mid_h) -> (out_w, out_h), up and down
TRIPLES = [((144, 81), (256, 144), (1920, 1080)), ((256, 144), (135, 76), (540, 304)), ((101, 37), (37, 101), (101, 37)),
           ((5, 3), (7, 4), (16, 9)), ((16, 9), (16, 9), (16, 9)), ((17, 9), (13, 5), (6, 4)), ((1024, 576), (512, 288), (1920, 1080)),
           ((37, 53), (101, 7), (64, 41)), ((3, 2), (1, 1), (9, 7)), ((1, 1), (4, 4), (3, 5))]


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "-".join(f"{w}x{h}" for w, h in t))
def test_composed_nearest_maps_equal_two_interpolates_on_index_ramps(triple):
    import torch
    import torch.nn.functional as TF
    (W, H), (mw, mh), (ow, oh) = triple
    ramp = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)                # (exact below 2^24)
    want = TF.interpolate(TF.interpolate(ramp, size=(mh, mw), mode="nearest"), size=(oh, ow), mode="nearest")[0, 0].numpy().astype(np.int64)
    sy, sx = vr.near_twice(H, mh, oh), vr.near_twice(W, mw, ow)
    assert np.array_equal(sy[:, None] * W + sx[None, :], want)
    mid = vr.nearest_planes(ramp.numpy()[0], (mw, mh))
    assert np.array_equal(mid, TF.interpolate(ramp, size=(mh, mw), mode="nearest")[0].numpy())
    codes, plane = vr.nearest_depth_codes(ramp.numpy()[0] / F(H * W), (mw, mh), (ow, oh), 1)
    assert codes.shape == (1, oh, ow, 3) and np.array_equal(plane[0], (want / F(H * W)).astype(F))


# ---- (c): the median ------------------------------------------------------------------------------------------------------------------
def _torch_median(cv, ref, mask):
    """video_mvsa.py:261-293 on one frame, by torch on the CPU -> (s, count)."""
    import torch
    import torch.nn.functional as TF
    d_ref = torch.from_numpy(np.asarray(ref, F))[None, None]
    d_cv = torch.from_numpy(np.asarray(cv, F))[None, None]
    h_cv, w_cv = d_cv.shape[-2:]
    d_ref_at_cv = TF.interpolate(d_ref, size=(h_cv, w_cv), mode="nearest")
    m = torch.from_numpy(np.asarray(mask)).to(torch.bool)[None, None] if mask is not None else (d_cv > 0)
    if m.shape[-2:] != (h_cv, w_cv):
        m = TF.interpolate(m.float(), size=(h_cv, w_cv), mode="nearest").to(torch.bool)
    valid = m & torch.isfinite(d_cv) & torch.isfinite(d_ref_at_cv) & (d_cv > 0) & (d_ref_at_cv > 0)
    num, den = d_cv[valid], d_ref_at_cv[valid] + 1e-6
    if num.numel() > 0:
        return F((num / den).clamp_min(0.0).median().item()), int(num.numel())
    return F(1.0), 0


def _median_case(rng, count, shape=(9, 14), ref_shape=None, mask_shape=None, equal=False, inf=False):
    """A frame with exactly `count` valid ratios."""
    h, w = shape
    cv = rng.uniform(0.1, 50.0, (h, w)).astype(F)
    ref = rng.uniform(0.1, 50.0, ref_shape or shape).astype(F)
    if equal:
        cv[...] = F(3.0)
        ref[...] = F(1.5)
    bad = rng.permutation(h * w)[count:]
    cv.reshape(-1)[bad] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, -np.inf, -0.0], F), bad.size)
    if inf and count:
        good = np.setdiff1d(np.arange(h * w), bad)
        cv.reshape(-1)[good[0]] = F(3e38)
        ys, xs = np.unravel_index(good[0], (h, w))
        ref[vr.near(ref.shape[0], h)[ys], vr.near(ref.shape[1], w)[xs]] = F(1e-3)      # 3e38 / 1e-3 overflows to +inf
    mask = None if mask_shape is None else np.ones(mask_shape, np.uint8)
    return cv, ref, mask


def test_median_restatement_equals_torch_median():
    rng = np.random.default_rng(2330)
    cases = [_median_case(rng, c) for c in (0, 1, 2, 3, 57, 58, 126)]
    cases += [_median_case(rng, 40, equal=True), _median_case(rng, 41, inf=True), _median_case(rng, 1, inf=True)]
    cases += [_median_case(rng, 77, ref_shape=(18, 28)), _median_case(rng, 90, ref_shape=(5, 9))]
    counts = [0, 1, 2, 3, 57, 58, 126, 40, 41, 1, 77, 90]
    for k, (cv, ref, mask) in enumerate(cases):
        med, cnt = vr.ratio_median(cv[None], ref[None])
        want, n = _torch_median(cv, ref, None)
        assert int(cnt[0]) == n == counts[k], (k, int(cnt[0]), n)
        assert med[0].view(np.uint32) == want.view(np.uint32), (k, med[0], want)
    assert np.isinf(vr.ratio_median(cases[9][0][None], cases[9][1][None])[0][0]), "a single ratio that overflows is the median: +inf"


def test_median_with_a_mask_at_another_size():
    rng = np.random.default_rng(2331)
    for mask_shape in ((9, 14), (4, 7), (18, 30), (1, 1)):
        cv, ref, _ = _median_case(rng, 100)
        mask = (rng.random(mask_shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, mask_shape).astype(np.uint8)
        med, cnt = vr.ratio_median(cv[None], ref[None], mask[None])
        want, n = _torch_median(cv, ref, mask)
        assert int(cnt[0]) == n and med[0].view(np.uint32) == want.view(np.uint32), mask_shape
    zero = np.zeros((3, 3), np.uint8)
    assert vr.ratio_median(cv[None], ref[None], zero[None])[0][0] == F(1) and _torch_median(cv, ref, zero) == (F(1), 0)


def test_the_lower_median_is_taken():
    cv = np.array([[1.0, 2.0, 3.0, 4.0]], F)
    ref = np.ones((1, 4), F)
    med, cnt = vr.ratio_median(cv[None], ref[None])
    assert cnt[0] == 4 and med[0] == F(2.0) / (F(1) + F(1e-6))


# ---- (d): the host logic --------------------------------------------------------------------------------------------------------------
def test_reference_indices_against_hand_written_lists(host):
    ri = host.reference_indices
    assert ri(0, 12, 7) == [1, 2, 3] and ri(1, 12, 7) == [0, 2, 3, 4] and ri(5, 12, 7) == [2, 3, 4, 6, 7, 8]
    assert ri(11, 12, 7) == [8, 9, 10] and ri(10, 12, 7) == [7, 8, 9, 11]
    assert ri(5, 12, 8) == [1, 2, 3, 4, 6, 7, 8, 9] and ri(0, 12, 8) == [1, 2, 3, 4], "an even window behaves as the next odd one"
    assert ri(5, 12, 1) == [4, 6] and ri(0, 12, 1) == [1] and ri(11, 12, 1) == [10], "--window 1 still takes one neighbour on each side"
    assert ri(5, 12, 2) == [4, 6] and ri(5, 12, 3) == [4, 6] and ri(5, 12, 0) == [4, 6]
    assert ri(0, 1, 7) == [0] and ri(0, 1, 1) == [0], "a one-frame clip refers to itself"
    assert ri(0, 2, 7) == [1] and ri(1, 2, 7) == [0] and ri(0, 2, 1) == [1] and ri(1, 2, 2) == [0]
    assert ri(1, 3, 8) == [0, 2]
    for n in (1, 2, 3, 12):
        for window in (0, 1, 2, 3, 7, 8):
            assert [ri(i, n, window) for i in range(n)] == [vr.reference_indices(i, n, window) for i in range(n)]
    assert [host.half_window(w) for w in (0, 1, 2, 3, 7, 8)] == [1, 1, 1, 1, 3, 4]


def test_the_three_forms_of_a_transformation_file(host, tmp_path):
    A = (np.arange(16, dtype=np.float64).reshape(4, 4) + 0.1).tolist()
    B = (np.eye(4) * 2).tolist()
    flat = [float(v) for v in np.arange(16)]
    eye = np.eye(4, dtype=F)

    def load(data, n):
        p = tmp_path / "t.json"
        p.write_text(json.dumps(data))
        T = host.load_transforms(str(p), n)
        assert T.dtype == np.float32 and T.shape == (n, 4, 4)
        return T
    T = load([A, B, flat], 4)                                       # a list of matrices: shorter than the clip, 16 flat values
    assert np.array_equal(T[0], np.array(A, F)) and np.array_equal(T[1], np.array(B, F)) and np.array_equal(T[2], np.arange(16, dtype=F).reshape(4, 4))
    assert np.array_equal(T[3], eye)
    assert load([A, B, flat], 2).shape == (2, 4, 4)                 # longer than the clip
    T = load([{"cam_T_world": A}, {"Tcw": B}, {"other": A}, 7], 4)  # a list of dicts; what names nothing stays the identity
    assert np.array_equal(T[0], np.array(A, F)) and np.array_equal(T[1], np.array(B, F)) and np.array_equal(T[2], eye) and np.array_equal(T[3], eye)
    T = load({"2": A, "0": {"cam_T_world": B}, "x": A, "9": A, "-1": A}, 3)     # a dict by frame number
    assert np.array_equal(T[2], np.array(A, F)) and np.array_equal(T[0], np.array(B, F)) and np.array_equal(T[1], eye)
    assert np.array_equal(host.load_transforms(None, 2), np.stack([eye, eye])) and np.array_equal(host.load_transforms("", 1), eye[None])
    for bad in ([[1, 2, 3]], [{"cam_T_world": [[1, 2], [3, 4]]}], {"0": [1.0] * 15}):
        p = tmp_path / "bad.json"
        p.write_text(json.dumps(bad))
        with pytest.raises(ValueError, match="4x4"):
            host.load_transforms(str(p), 2)
        with pytest.raises(ValueError, match="4x4"):
            host.check_transformation_file(str(p))


def test_model_size_rounds_halves_as_python_does(host):
    assert host.model_size(1920, 1080, 1024)[:2] == (1024, 576) and host.model_size(960, 540, 1024)[:2] == (1024, 576)
    assert host.model_size(4, 3, 2)[:2] == (2, 2) and host.model_size(4, 5, 2)[:2] == (2, 2) and host.model_size(4, 7, 2)[:2] == (2, 4)
    assert host.model_size(4, 1, 2)[:2] == (2, 0), "0.5 rounds to 0: the tool refuses the size"
    assert host.model_size(64, 36, 48) == (48, 27, 0.75) and host.model_size(3, 2, 1024)[:2] == (1024, 683)


def test_intrinsics_are_the_references_calls(host):
    import torch
    from metric_depth_video_toolbox_amd.depth_map_tools import compute_camera_matrix
    K44, invK44, K44_s, invK44_s = host.intrinsics(60.0, None, 64, 36, 48)
    cam = compute_camera_matrix(60.0, None, 64, 36)
    want = torch.eye(4, dtype=torch.float32)
    want[:3, :3] = torch.from_numpy(cam).float()
    S = torch.tensor([[0.75, 0, 0, 0], [0, 0.75, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    assert all(t.dtype == torch.float32 and t.shape == (4, 4) and t.device.type == "cpu" for t in (K44, invK44, K44_s, invK44_s))
    assert torch.equal(K44, want) and torch.equal(invK44, torch.inverse(want))
    assert torch.equal(K44_s, S @ want) and torch.equal(invK44_s, torch.inverse(S @ want))
    assert float(K44_s[0, 2]) == 24.0 and float(K44_s[1, 2]) == 13.5 and float(K44[0, 0]) == float(np.float32(cam[0, 0]))
    assert float(host.intrinsics(None, 40.0, 64, 36, 48)[0][1, 1]) == float(np.float32(compute_camera_matrix(None, 40.0, 64, 36)[1, 1]))


def test_the_parsers_defaults_are_the_references(host):
    a = host.build_parser().parse_args(["--color_video", "x.mkv"])
    assert (a.color_video, a.xfov, a.yfov, a.transformation_file, a.max_frames, a.window, a.resize_w) == ("x.mkv", None, None, None, -1, 7, 1024)
    assert (a.fast_cost_volume, a.max_depth, a.apply_cost_volume_scale, a.save_cost_volume_scales) == (False, 100, False, False)
    assert (a.batch, a.generator, a.video_decoder, a.video_encoder) == (8, "mvsanywhere", "host", "host")
    assert host.output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_cv_scales.json")
    assert host.output_paths("x.npy", False) == ("x.npy_tmp_depth.npy", "x.npy_depth.npy", "x.npy_depth.npy_cv_scales.json")
    assert [host.frames_to_read(12, m) for m in (-1, 0, 5, 12, 40)] == [12, 12, 5, 12, 12]
    with pytest.raises(ValueError, match="pkg.module:callable"):
        host.load_generator("nothing")
    with pytest.raises(RuntimeError, match="needs the mvsanywhere package"):
        host.load_generator("mvsanywhere")


def test_refusals_name_their_reason_and_write_nothing(host, tool, tmp_path):
    clip = tmp_path / "clip.npy"
    np.save(clip, np.zeros((2, 4, 6, 3), np.uint8))
    before = sorted(os.listdir(tmp_path))

    def infer(*a):
        raise AssertionError("the model is not reached")
    args = host.build_parser().parse_args(["--color_video", str(clip)])
    with pytest.raises(ValueError, match="--xfov or --yfov is required"):
        tool.run(args, infer)
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps([np.eye(4).tolist(), [[1, 2, 3], [4, 5, 6]]]))
    before.append("bad.json")
    args = host.build_parser().parse_args(["--color_video", str(clip), "--xfov", "60", "--transformation_file", str(bad)])
    with pytest.raises(ValueError, match="transformation 1 is not 4x4"):
        tool.run(args, infer)
    for flags in (["--batch", "0"], ["--resize_w", "0"]):
        with pytest.raises(ValueError, match="must be at least 1"):
            tool.run(host.build_parser().parse_args(["--color_video", str(clip), "--xfov", "60"] + flags), infer)
    assert sorted(os.listdir(tmp_path)) == sorted(before)


# ---- (e): the header and its binding ------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_by_both_libraries_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(HEADER)
    assert sorted(decls) == sorted(_lib.MVSA_SYMBOLS) == NAMES
    L, T = _lib.load(), ctypes.CDLL(_lib.lib_path("tuning"))
    main_header = open(os.path.join(REPO, "include", "mdvt.h")).read()
    api_unit = open(os.path.join(CSRC, "mdvt_api.hip")).read()
    own_unit = open(os.path.join(CSRC, "mdvt_api_mvsa.hip")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    others = (_lib.SYMBOLS + _lib.DECODE_SYMBOLS + _lib.STREAM_DECODE_SYMBOLS + _lib.CONVERGENCE_SYMBOLS + _lib.METRIC_ALIGN_SYMBOLS +
              _lib.DEPTH_SINK_SYMBOLS + _lib.DEPTH_ENGINE_SYMBOLS + _lib.INFILL_ADAPTER_SYMBOLS + _lib.INFILL_ENGINE_SYMBOLS + _lib.VIEW_SYMBOLS +
              _lib.GEOMETRY_SYMBOLS + _lib.VIDEO_MASK_SYMBOLS)
    for name, args in decls.items():
        assert hasattr(L, name) and hasattr(T, name), name
        assert name not in others and name not in main_header
        assert not re.search(r"^int " + name + r"\(", api_unit, flags=re.M) and re.search(r"^int " + name + r"\(", own_unit, flags=re.M)
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in args.split(",")]
        assert getattr(L, name).argtypes == want and getattr(L, name).restype is ctypes.c_int, name
        assert args.startswith("mdvt_ctx* ctx,") and args.endswith("void* stream")
        for a in args.split(","):                                   # pitches and strides are 64-bit
            if re.search(r"(pitch|stride)$", a.strip()):
                assert a.split()[0] == "size_t", a
    assert L.mdvt_version() == 15                                   # include/mdvt.h is unchanged
    text = open(HEADER).read()
    for cited in ("video_mvsa.py:59-63", "video_mvsa.py:268", "video_mvsa.py:261-293", "video_mvsa.py:297"):
        assert cited in text, f"the header cites {cited}"


def test_a_null_context_is_refused_without_a_device():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert L.mdvt_bilinear_model_frames(None, 4, 4, 1, None, 12, 48, 0, 2, 2, None, 8, 16, 48, None) == -1
    assert L.mdvt_nearest_depth_codes(None, 4, 4, 1, None, 16, 64, 2, 2, None, 0, 100.0, 8, 8, None, 24, 192, 0, None, 32, 256, None) == -1
    assert L.mdvt_ratio_median(None, 1, 4, 4, None, 16, 64, 4, 4, None, 16, 64, 4, 4, None, 4, 16, None, None, None) == -1


def test_the_package_module_takes_no_address(host):
    src = open(host.__file__).read()
    assert "data_ptr" not in src and "UNTESTED" in src
