"""The mask-video step, host side -- no GPU: the restatement of Pillow's 8-bit Lanczos resize (tests/video_mask_ref.py) against Pillow
itself and against tests/golden/video_mask.npz (recorded from Pillow by tests/golden/gen_video_mask_golden.py), the library's own table
builder (csrc/mdvt_lanczos_table.h in a program of its own, plain and under the sanitizers) against the restatement's tables, the new
header and its binding, the parser, the file names, --max_frames, the refusals, and the two normalisations against the literal NumPy
expressions of rembg's source."""
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
import video_mask_ref as vr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdvt_video_mask.h")
GOLDEN = os.path.join(REPO, "tests", "golden", "video_mask.npz")
CSRC = os.path.join(REPO, "metric_depth_video_toolbox_amd", "csrc")
F = np.float32
NAMES = ["mdvt_lanczos_resize_u8", "mdvt_mask_from_prediction", "mdvt_mask_model_input"]

# the cases the restatement was first held to Pillow on: RGB to the network's square, L from it; then one enlarging RGB and one shrinking L
RGB_SOURCES = [(1, 1), (5, 4), (37, 23), (64, 48), (333, 187), (641, 321), (320, 200), (320, 320), (1920, 1080)]
L_TARGETS = [(1, 1), (5, 4), (37, 23), (320, 200), (641, 361), (1000, 7), (1920, 1080)]
PIL_CASES = [("RGB", s, (320, 320)) for s in RGB_SOURCES] + [("L", (320, 320), t) for t in L_TARGETS] + \
            [("RGB", (5, 4), (16, 12)), ("L", (50, 40), (21, 13))]


def _content(kind, mode, size, seed):
    rng = np.random.default_rng(seed)
    shape = (size[1], size[0]) + ((3,) if mode == "RGB" else ())
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    b = max(1, min(size) // 6)                                     # 0/255 in blocks: edges, whose overshoot reaches both clamps
    cells = rng.integers(0, 2, (-(-size[1] // b), -(-size[0] // b)) + shape[2:]) * 255
    return np.repeat(np.repeat(cells, b, axis=0), b, axis=1)[:size[1], :size[0]].astype(np.uint8)


def _tool():
    spec = importlib.util.spec_from_file_location("generate_video_mask_tool", os.path.join(REPO, "tools", "generate_video_mask.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def host():
    from metric_depth_video_toolbox_amd import video_mask
    return video_mask


# ---- (a), (b): the restatement is Pillow's resize ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PIL_CASES, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-to-{c[2][0]}x{c[2][1]}")
def test_the_restatement_equals_pillow_byte_for_byte(case):
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("PILLOW IS NOT IMPORTABLE HERE: the restatement is held to the recorded bytes of tests/golden/video_mask.npz only")
    mode, src, dst = case
    for k, kind in enumerate(("noise", "step")):
        img = _content(kind, mode, src, 7000 + 2 * PIL_CASES.index(case) + k)
        want = np.asarray(Image.fromarray(img, mode).resize(dst, Image.LANCZOS))
        got = vr.lanczos_resize(img, dst, 3 if mode == "RGB" else 1)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert int((got != want).sum()) == 0, f"{mode} {src} -> {dst}, {kind}: {int((got != want).sum())} bytes differ from Pillow's"
        if kind == "step" and min(src) > 4 and min(dst) > 4 and src != dst:
            assert want.min() == 0 and want.max() == 255            # the steps reach both clamps


def test_the_restatement_equals_the_bytes_recorded_from_pillow():
    golden = dict(np.load(GOLDEN))
    assert str(golden.pop("pillow_version")).startswith("12.")
    keys = sorted(k[:-3] for k in golden if k.endswith("_in"))
    assert len(keys) == 28 and os.path.getsize(GOLDEN) < 200 << 10
    kinds = set()
    for key in keys:
        mode, src, _to, dst, kind = key.split("_")
        dst = tuple(int(v) for v in dst.split("x"))
        src = tuple(int(v) for v in src.split("x"))
        img, want = golden[key + "_in"], golden[key + "_out"]
        assert img.shape[:2] == (src[1], src[0]) and want.shape[:2] == (dst[1], dst[0])
        got = vr.lanczos_resize(img, dst, 3 if mode == "RGB" else 1)
        assert np.array_equal(got, want), key
        kinds.add((mode, src[0] < dst[0], src[1] < dst[1], src[0] == dst[0] or src[1] == dst[1]))
    # both modes; both axes enlarging, both shrinking, one each way, a skipped pass
    assert {k[0] for k in kinds} == {"RGB", "L"} and any(k[1] and k[2] for k in kinds) and any(not (k[1] or k[2] or k[3]) for k in kinds)
    assert any(k[1] != k[2] and not k[3] for k in kinds) and any(k[3] for k in kinds)


def test_equal_sizes_are_a_copy_and_a_pass_alone_leaves_the_other_axis():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(vr.lanczos_resize(img, (13, 9), 3), img)
    only_rows = vr.lanczos_resize(img, (13, 4), 3)
    assert np.array_equal(only_rows, vr._pass(img, 4, 0)) and only_rows.shape == (4, 13, 3)
    # channels are independent, and a batch is its frames
    assert np.array_equal(vr.lanczos_resize(img, (5, 7), 3)[..., 1], vr.lanczos_resize(np.ascontiguousarray(img[..., 1]), (5, 7), 1))
    both = vr.lanczos_resize(np.stack([img, img[::-1]]), (5, 7), 3)
    assert np.array_equal(both[1], vr.lanczos_resize(np.ascontiguousarray(img[::-1]), (5, 7), 3))


# ---- the library's table builder, in a program of its own ----------------------------------------------------------------------------
TABLE_PAIRS = [(1, 1), (1, 7), (7, 1), (5, 320), (23, 320), (1920, 320), (1080, 320), (320, 1920), (320, 1080), (320, 361), (333, 320),
               (8192, 1), (8192, 8191), (4097, 4096), (2160, 320), (8193, 4), (0, 4)]


def _build_table_program(sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        return None, "no g++"
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="lanczos_table_"), "lanczos_table_host_asan" if sanitize else "lanczos_table_host")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
           os.path.join(REPO, "tests", "lanczos_table_host.cpp")]
    if sanitize:
        cmd[3:3] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode and sanitize and any(t in r.stderr for t in ("cannot find -lasan", "cannot find -lubsan", "libasan.a", "libubsan.a", "unrecognized")):
        return None, r.stderr[-400:]
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_the_librarys_tables_equal_the_restatements(sanitize, tmp_path):
    exe, why = _build_table_program(sanitize)
    if exe is None:
        pytest.skip(why)
    res = str(tmp_path / "tables.bin")
    r = subprocess.run([exe, res] + [str(v) for p in TABLE_PAIRS for v in p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    words = np.fromfile(res, np.int32)
    at = 0
    for n_in, n_out in TABLE_PAIRS:
        ok, a, b, ksize = (int(v) for v in words[at:at + 4])
        at += 4
        assert (a, b) == (n_in, n_out)
        if not 1 <= n_in <= 8192 or not 1 <= n_out <= 8192:
            assert ok == 0                                          # beyond the size limit: no table
            continue
        bounds, k = vr.lanczos_table(n_in, n_out)
        assert ok == 1 and ksize == k.shape[1], (n_in, n_out)
        assert np.array_equal(words[at:at + 2 * n_out].reshape(n_out, 2), bounds), (n_in, n_out)
        at += 2 * n_out
        assert np.array_equal(words[at:at + ksize * n_out].reshape(ksize, n_out).T, k), (n_in, n_out)      # the library stores tap-major
        at += ksize * n_out
        assert (bounds[:, 0] + bounds[:, 1]).max() <= n_in and bounds.min() >= 0 and bounds[:, 1].max() <= ksize
    assert at == words.size


# ---- (c): the header and its binding ---------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_by_both_libraries_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(HEADER)
    assert sorted(decls) == sorted(_lib.VIDEO_MASK_SYMBOLS) == NAMES
    L, T = _lib.load(), ctypes.CDLL(_lib.lib_path("tuning"))
    main_header = open(os.path.join(REPO, "include", "mdvt.h")).read()
    api_unit = open(os.path.join(CSRC, "mdvt_api.hip")).read()
    own_unit = open(os.path.join(CSRC, "mdvt_api_video_mask.hip")).read()
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    others = (_lib.SYMBOLS + _lib.DECODE_SYMBOLS + _lib.STREAM_DECODE_SYMBOLS + _lib.CONVERGENCE_SYMBOLS + _lib.METRIC_ALIGN_SYMBOLS +
              _lib.DEPTH_SINK_SYMBOLS + _lib.DEPTH_ENGINE_SYMBOLS + _lib.INFILL_ADAPTER_SYMBOLS + _lib.INFILL_ENGINE_SYMBOLS + _lib.VIEW_SYMBOLS +
              _lib.GEOMETRY_SYMBOLS)
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
    assert (_lib.LANCZOS_AUTO, _lib.LANCZOS_FUSED, _lib.LANCZOS_TWO_LAUNCH) == (0, 1, 2)
    text = open(HEADER).read()
    for k, v in (("MDVT_LANCZOS_AUTO", 0), ("MDVT_LANCZOS_FUSED", 1), ("MDVT_LANCZOS_TWO_LAUNCH", 2)):
        assert re.search(rf"#define {k} {v}\b", text)


def test_a_null_context_is_refused_without_a_device():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert L.mdvt_lanczos_resize_u8(None, 4, 4, 3, 1, None, 12, 48, 2, 2, None, 6, 12, 0, None, None) == -1
    assert L.mdvt_mask_model_input(None, 4, 4, 1, None, 12, 48, 0, 2, 2, None, None, None, 8, 16, 48, None) == -1
    assert L.mdvt_mask_from_prediction(None, 4, 4, 1, None, 16, 64, 2, 2, 1, None, 2, 4, None) == -1


# ---- (d): parser, names, lists, --max_frames, refusals ---------------------------------------------------------------------------------
def test_the_parsers_defaults_are_the_references(host):
    a = host.build_parser().parse_args(["--color_video", "x.mkv"])
    assert (a.color_video, a.max_frames, a.batch_size) == ("x.mkv", -1, 8)
    assert (a.model_size, a.generator, a.video_decoder, a.video_encoder) == (320, "rembg_u2net", "host", "host")
    host.check_flags(a)
    with pytest.raises(SystemExit):
        host.build_parser().parse_args([])                           # --color_video is required
    a = host.build_parser().parse_args(["--color_video", "x", "--max_frames", "5", "--batch_size", "3", "--model_size", "64",
                                        "--video_decoder", "device_all", "--video_encoder", "device", "--generator", "m:f"])
    assert (a.max_frames, a.batch_size, a.model_size, a.video_decoder, a.video_encoder, a.generator) == (5, 3, 64, "device_all", "device", "m:f")
    assert (host.U2NET_MEAN, host.U2NET_STD, host.U2NET_SIZE) == (vr.U2NET_MEAN, vr.U2NET_STD, vr.U2NET_SIZE[0])
    assert vr.U2NET_MEAN == (0.485, 0.456, 0.406) and vr.U2NET_STD == (0.229, 0.224, 0.225) and host.DEFAULT_FPS == 30.0


def test_file_names_lists_and_max_frames(host, tmp_path):
    assert host.output_paths("x.mkv") == ("x.mkv_tmp_mask.mkv", "x.mkv_mask.mkv")
    assert host.output_paths("x.npy", video=False) == ("x.npy_tmp_mask.npy", "x.npy_mask.npy")
    lst = tmp_path / "clips.txt"
    lst.write_text("# a list\n\n a.mkv \nb.mkv\n")
    assert host.clips_from_argument(str(lst)) == ["a.mkv", "b.mkv"] and host.clips_from_argument("a.mkv") == ["a.mkv"]

    def reference_loop(n_in_file, max_frames):                       # gvm:85-109 as written
        frame_n, written = 0, 0
        for _ in range(n_in_file):
            frame_n += 1
            if max_frames != -1 and frame_n > max_frames:
                break
            written += 1
        return written
    for n in (1, 5, 12):
        for m in (-1, 0, 1, 4, 5, 6, 12, 13, 100):
            assert host.frames_to_write(n, m) == reference_loop(n, m), (n, m)
    # the tmp -> final step: renamed when the frame count is right, removed when the loop fails
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    tmp, final = host.output_paths(str(tmp_path / "c.npy"), video=False)
    with ClipOutput(tmp, final, 2, (2, 3, 3)) as out:
        assert os.path.exists(tmp) and not os.path.exists(final)
        out.arr[...] = 255
    assert os.path.exists(final) and not os.path.exists(tmp) and np.load(final).shape == (2, 2, 3, 3)


@pytest.mark.parametrize("flags,error,text", [
    (["--batch_size", "0"], ValueError, "--batch_size"), (["--model_size", "0"], ValueError, "--model_size"),
    (["--model_size", "8193"], ValueError, "--model_size"), (["--max_frames", "-2"], ValueError, "--max_frames"),
    (["--generator", "not_a_spec"], ValueError, "--generator"), (["--generator", "json:no_such_callable"], ValueError, "no callable"),
    ([], Exception, "input color_video does not exist"), (["--video_decoder", "device"], Exception, "input color_video does not exist")])
def test_refusals_come_before_anything_is_written(host, tmp_path, flags, error, text):
    tool = _tool()
    missing = str(tmp_path / "no_such_clip.mkv")
    argv = ["--color_video", missing] + (flags if "--generator" in flags else flags + ["--generator", "json:dumps"])
    with pytest.raises(error, match=text):
        tool.run(host.build_parser().parse_args(argv))
    assert os.listdir(tmp_path) == []


def test_a_dump_of_the_wrong_kind_and_an_empty_count_are_refused_and_leave_nothing(host, tmp_path):
    tool = _tool()
    planes = str(tmp_path / "planes.npy")
    np.save(planes, np.zeros((3, 4, 5), np.uint8))
    frames = str(tmp_path / "frames.npy")
    np.save(frames, np.zeros((3, 4, 5, 3), np.uint8))
    before = sorted(os.listdir(tmp_path))
    for argv, text in ((["--color_video", planes], r"uint8 \[N, H, W, 3\]"), (["--color_video", frames, "--max_frames", "0"], "No frames read"),
                       (["--color_video", frames, "--video_encoder", "device"], "video_encoder"),
                       (["--color_video", frames, "--video_decoder", "device"], "video_decoder")):
        with pytest.raises(ValueError, match=text):
            tool.run(host.build_parser().parse_args(argv + ["--generator", "json:dumps"]))
        assert sorted(os.listdir(tmp_path)) == before
    lst = tmp_path / "clips.txt"
    lst.write_text(str(tmp_path / "gone.mkv") + "\n")
    with pytest.raises(Exception, match="input color_video does not exist"):
        tool.run(host.build_parser().parse_args(["--color_video", str(lst), "--generator", "json:dumps"]))
    assert sorted(os.listdir(tmp_path)) == sorted(before + ["clips.txt"])


def test_the_default_generator_fails_with_one_line_where_its_packages_are_missing(host, monkeypatch):
    import json
    for gone in ("rembg", "onnxruntime"):
        with monkeypatch.context() as m:
            m.setitem(sys.modules, gone, None)                      # (an import of it raises ImportError, installed or not)
            if gone == "onnxruntime":
                m.setitem(sys.modules, "rembg", type(sys)("rembg"))
            for spec in (None, "rembg_u2net"):
                with pytest.raises(RuntimeError, match="rembg and onnxruntime") as e:
                    host.load_generator(spec)
                assert "\n" not in str(e.value)
    assert host.load_generator("json:dumps") is json.dumps
    assert "UNTESTED" in host.RembgU2NetGenerator.__doc__
    src = open(os.path.join(REPO, "metric_depth_video_toolbox_amd", "video_mask.py")).read()
    assert "data_ptr" not in src and not re.search(r"^import (rembg|onnxruntime)|^from (rembg|onnxruntime)", src, flags=re.M)


# ---- (e): the two normalisations are rembg's expressions ---------------------------------------------------------------------------------
def _rembg_normalize(im, mean, std):
    """sessions/base.py: normalize, from `im_ary = np.array(im)` on (im: the resized RGB image)."""
    im_ary = np.array(im)
    im_ary = im_ary / max(np.max(im_ary), 1e-6)
    tmpImg = np.zeros((im_ary.shape[0], im_ary.shape[1], 3))
    tmpImg[:, :, 0] = (im_ary[:, :, 0] - mean[0]) / std[0]
    tmpImg[:, :, 1] = (im_ary[:, :, 1] - mean[1]) / std[1]
    tmpImg[:, :, 2] = (im_ary[:, :, 2] - mean[2]) / std[2]
    tmpImg = tmpImg.transpose((2, 0, 1))
    return np.expand_dims(tmpImg, 0).astype(np.float32)


def test_the_model_input_is_rembgs_normalize():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (3, 23, 37, 3), dtype=np.uint8)
    frames[1] //= 3                                                  # a maximum below 255
    frames[2] = 0                                                    # max(np.max, 1e-6)
    assert (np.zeros(2, np.uint8) / np.uint8(3)).dtype == np.float64     # NumPy's uint8 / uint8
    for size, mean, std in (((16, 12), vr.U2NET_MEAN, vr.U2NET_STD), ((37, 23), (0.5, 0.5, 0.5), (1.0, 1.0, 1.0))):
        got = vr.mask_model_input(frames, size, mean, std)
        for n in range(3):
            im = vr.lanczos_resize(frames[n], size, 3)
            assert np.array_equal(got[n:n + 1].view(np.uint32), _rembg_normalize(im, mean, std).view(np.uint32)), (size, n)
        assert np.array_equal(vr.mask_model_input(frames[..., ::-1], size, mean, std, bgr=True).view(np.uint32), got.view(np.uint32))
    zero = vr.mask_model_input(frames[2:], (16, 12))
    assert np.array_equal(zero[0, 0], np.full((12, 16), F((0.0 / 1e-6 - 0.485) / 0.229)))
    assert frames[1].max() < 255 and vr.lanczos_resize(frames[1], (16, 12), 3).max() < 255


def _rembg_predict_tail(pred, size):
    """sessions/u2net.py: predict, from `pred = ort_outs[0][:, 0, :, :]` to the mask's resize (by the restatement)."""
    ma = np.max(pred)
    mi = np.min(pred)
    pred = (pred - mi) / (ma - mi)
    pred = np.squeeze(pred)
    return vr.lanczos_resize((pred * 255).astype("uint8"), size, 1)


def test_the_mask_is_rembgs_predict_tail_and_the_writers_frame():
    rng = np.random.default_rng(12)
    pred = rng.normal(0.4, 0.5, (4, 20, 24)).astype(F)               # outside [0, 1]
    pred[1] = 1 / (1 + np.exp(-4 * pred[1]))                         # a sigmoid's range
    pred[2] *= F(1e-3)
    pred[3, 0, :3] = [-0.0, 0.0, -7.5]
    for size in ((24, 20), (9, 7), (31, 40)):
        got = vr.mask_from_prediction(pred, size)
        for n in range(4):
            assert np.array_equal(got[n], _rembg_predict_tail(pred[n:n + 1], size)), (size, n)
        three = vr.mask_from_prediction(pred, size, channels=3)
        assert three.shape == got.shape + (3,) and all(np.array_equal(three[..., c], got) for c in range(3))
    assert vr.prediction_bytes(pred).min() == 0 and vr.prediction_bytes(pred).max() == 255
    # save_grayscale_video's frame with max_depth 255 (dfh:221-230) is the identity on all 256 values
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal((np.clip(v, 0, 255.0) / 255.0 * 255.0).astype(np.uint8), v)
    # the decrees: a constant plane, a NaN, an infinity and an infinite range give an all-zero mask
    bad = np.ones((4, 5, 6), F)
    bad[1, 2, 3], bad[2, 0, 0] = np.nan, np.inf
    bad[3, 0, :2] = [-3e38, 3e38]
    assert not vr.mask_from_prediction(bad, (8, 4)).any()
