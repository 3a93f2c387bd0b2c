"""The infill adapter's host side -- no GPU: the binding of the four entry points of include/mdvt_infill_adapter.h, the restated
colour match of tests/infill_adapter_ref.py against the reference's own outputs (tests/golden/lhm_transfer_*.npz), the u8 resize
rule against hand-computed values, the chunk schedule against a literal model of the reference's loop, and the command line's
refusals."""
import hashlib
import os
import re

import numpy as np
import pytest

import infill_adapter_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = R.GOLDENS
NAMES = ["mdvt_adapter_composite_eye", "mdvt_adapter_prepare_eye", "mdvt_lhm_apply", "mdvt_lhm_moments"]


def test_the_entry_points_are_exported_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "mdvt_infill_adapter.h")).read()
    declared = sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert declared == sorted(_lib.INFILL_ADAPTER_SYMBOLS) == NAMES
    others = _lib.SYMBOLS + _lib.DECODE_SYMBOLS + _lib.CONVERGENCE_SYMBOLS + _lib.METRIC_ALIGN_SYMBOLS
    main = open(os.path.join(REPO, "include", "mdvt.h"), "rb").read()
    for s in NAMES:
        assert hasattr(L, s) and s not in others and s.encode() not in main
    # include/mdvt.h is byte for byte what ABI 0.15 shipped
    assert hashlib.sha256(main).hexdigest() == "5f1d16f6a06b01ef262e293213d5ed895e2c27a0172feeb538a2b486b3720e04"
    assert L.mdvt_version() == 15
    for doc in ("RESTATED, not observed", "single_precision=False", "3.2 %", "Footprint", "No byte parity with cv2"):
        assert doc in hdr
    # the argument counts of the binding are the header's
    body = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for s in NAMES:
        args = re.search(s + r"\s*\((.*?)\)\s*;", body, flags=re.S).group(1)
        assert len(getattr(L, s).argtypes) == args.count(",") + 1, s


# ---- the colour match against the reference's outputs ---------------------------------------------------------------------------

def test_the_goldens_cover_the_cases():
    names = {os.path.basename(p)[len("lhm_transfer_"):-4] for p in GOLDENS}
    assert names == {"48x64", "5x7", "constant", "few_kept", "crop96x128"}
    z = np.load(os.path.join(REPO, "tests", "golden", "lhm_transfer_few_kept.npz"))
    assert [int((m == 0).sum()) for m in z["mask"]] == [0, 2, 3]
    z = np.load(os.path.join(REPO, "tests", "golden", "lhm_transfer_constant.npz"))
    assert len(np.unique(z["video"][0].reshape(-1, 3), axis=0)) == 1
    for p in GOLDENS:
        assert os.path.getsize(p) < (1 << 20)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[13:-4] for p in GOLDENS])
def test_restated_colour_match_equals_the_reference_in_float64(path):
    z = np.load(path)
    got, pre = R.transfer_lhm(z["video"], z["reference"], z["mask"], want_pre=True)
    R.check_against_golden(got, z, os.path.basename(path))
    assert np.abs(pre - z["pre_f64"]).max() < 1e-9              # the two float64 routes (exact moments / centred products) agree far below a half


def test_module_algebra_is_the_restated_algebra():
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    z = np.load(os.path.join(REPO, "tests", "golden", "lhm_transfer_few_kept.npz"))
    mx, mr, ma = R.moments(z["video"]), R.moments(z["reference"], z["mask"]), R.moments(z["reference"])
    got = sci.lhm_params(np.array(mx, dtype=np.int64), np.array(mr, dtype=np.int64), np.array(ma, dtype=np.int64))
    for k in range(len(mx)):
        assert np.array_equal(got[k].view(np.uint64), R.lhm_params(mx[k], mr[k], ma[k]).view(np.uint64))
    big = [1024 * 768] + [255 * 1024 * 768] * 3 + [255 * 255 * 1024 * 768] * 6          # sums past 2^32: Python integers, not int64 products
    p = sci.lhm_params(np.array([big], dtype=np.int64), np.array([big], dtype=np.int64), np.array([big], dtype=np.int64))[0]
    assert np.array_equal(p[9:], [255.0] * 6) and np.allclose(p[:9].reshape(3, 3), np.eye(3), atol=1e-12)


# ---- the resize rule --------------------------------------------------------------------------------------------------------------

def test_resize_equal_sizes_copy_and_constants_stay():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    b = R.resize_u8(a, 13, 9)
    assert np.array_equal(a, b) and b is not a
    for v in (0, 1, 127, 200, 255):
        c = np.full((12, 16, 3), v, dtype=np.uint8)
        for ow, oh in ((7, 5), (40, 31), (8, 6), (16, 5), (3, 12)):
            assert (R.resize_u8(c, ow, oh) == v).all(), (v, ow, oh)


def test_resize_exact_half_is_the_area_mean():
    a = np.array([[0, 1, 10, 20], [2, 3, 30, 41], [255, 255, 7, 8], [255, 254, 9, 9]], dtype=np.uint8)
    # (0+1+2+3+2)>>2 = 2, (10+20+30+41+2)>>2 = 25, (1019+2)>>2 = 255, (33+2)>>2 = 8
    assert R.resize_u8(a, 2, 2).tolist() == [[2, 25], [255, 8]]
    # half in one axis only is the linear rule: columns 0,1 -> f = 0.5, weights 1024 / 1024; rows copy (weights 2048 / 0)
    assert R.resize_u8(a, 2, 4)[0].tolist() == [(((2048 * ((0 * 1024 + 1 * 1024) >> 4)) >> 16) + 2) >> 2, (((2048 * ((10 * 1024 + 20 * 1024) >> 4)) >> 16) + 2) >> 2]


def test_resize_hand_computed_values():
    """7 x 5 -> 16 x 12 and 16 x 12 -> 7 x 5 at the first, a middle and the last column and row.
    Up, columns (ratio 7/16): dx 0: f = -0.28125 -> sx 0, weights 2048 / 0; dx 8: f = 3.21875 -> sx 3, 1600 / 448; dx 15: f = 6.28125
    -> sx 6 (clamped), 2048 / 0.  Rows (ratio 5/12): dy 0: f = -0.2916667 -> sy -1, fraction 0.7083333 kept: 597 / 1451 on rows 0, 0;
    dy 6: f = 2.2083333 -> rows 2, 3, 1621 / 427; dy 11: f = 4.2916665 -> rows 4, 4, 1451 / 597.
    E.g. (dx 8, dy 6): h0 = 160 * 1600 + 197 * 448 = 344256, h1 = 215 * 1600 + 252 * 448 = 456896;
    ((1621 * 21516) >> 16) + ((427 * 28556) >> 16) + 2 = 532 + 186 + 2 = 720; 720 >> 2 = 180.
    Down, columns (ratio 16/7): dx 0: f = 0.6428572 -> 0, 1 with 731 / 1317; dx 3: f = 7.5 -> 7, 8 with 1024 / 1024; dx 6: f = 14.357143
    -> 14, 15 with 1317 / 731.  Rows (ratio 12/5): dy 0: f = 0.7 -> 0, 1 with 614 / 1434; dy 2: f = 5.5 -> 5, 6 with 1024 / 1024;
    dy 4: f = 10.3 -> 10, 11 with 1434 / 614.
    E.g. (dx 3, dy 2): h0 = (124 + 152) * 1024 = 282624, h1 = (222 + 253) * 1024 = 486400; ((1024 * 17664) >> 16) + ((1024 * 30400) >> 16)
    + 2 = 276 + 475 + 2 = 753; 753 >> 2 = 188."""
    y, x = np.mgrid[0:5, 0:7]
    small = ((37 * x + 11 * y * y + 5) % 256).astype(np.uint8)
    up = R.resize_u8(small, 16, 12)
    assert up.shape == (12, 16)
    assert [[int(up[dy, dx]) for dx in (0, 8, 15)] for dy in (0, 6, 11)] == [[5, 124, 227], [60, 180, 26], [181, 44, 147]]
    y, x = np.mgrid[0:12, 0:16]
    big = ((13 * x + 7 * y * y + 3 * x * y + 9) % 256).astype(np.uint8)
    down = R.resize_u8(big, 7, 5)
    assert down.shape == (5, 7)
    assert [[int(down[dy, dx]) for dx in (0, 3, 6)] for dy in (0, 2, 4)] == [[23, 127, 167], [113, 188, 134], [193, 148, 76]]
    # channels are independent
    rgb = np.stack([small, small[::-1], small[:, ::-1]], axis=-1)
    out = R.resize_u8(np.ascontiguousarray(rgb), 16, 12)
    for c in range(3):
        assert np.array_equal(out[..., c], R.resize_u8(np.ascontiguousarray(rgb[..., c]), 16, 12))
    assert R.taps(16, 7, True)[2][8] == 1600 and R.taps(12, 5, False)[3][0] == 1451


def test_gaussian_weights():
    w = R.gauss15()
    assert w.dtype == np.float32 and np.array_equal(w, w[::-1]) and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    assert abs(float(w[7]) / float(w[6]) - np.exp(1 / (2 * 2.6 * 2.6))) < 1e-6
    one = R.gauss_blur15(np.ones((9, 11), dtype=np.float32))
    assert np.abs(one - 1).max() < 1e-6                           # the reflected border loses no weight


# ---- the chunk schedule -----------------------------------------------------------------------------------------------------------

def literal_model(n_frames):
    """The reference's loop (scr:218-266) on frame numbers: -> (frames in the order they are written, [(first, last, len(buffer))])."""
    written, calls = [], []
    frame_buffer, first_chunk = [], True

    def deal(keep_first_three, chunk, keep_last_three):
        start = 0 if keep_first_three else 3
        end = len(chunk) if keep_last_three else len(chunk) - 3
        calls.append((keep_first_three, keep_last_three, len(chunk)))
        written.extend(chunk[start:end])

    for frame in range(n_frames):
        frame_buffer.append(frame)
        if len(frame_buffer) >= 25:
            deal(first_chunk, frame_buffer, False)
            first_chunk = False
            frame_buffer = frame_buffer[-6:]
    deal(first_chunk, frame_buffer, True)
    return written, calls


@pytest.mark.parametrize("n", [1, 6, 24, 25, 26, 44, 45, 63])
def test_schedule_writes_every_frame_once_in_order(n, orc):
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    written, calls = literal_model(n)
    assert written == list(range(n))
    sched = sci.chunk_schedule(n)
    assert [(f, l, held) for f, l, _, held, _ in sched] == calls
    got = [t for _, _, _, _, (a, b) in sched for t in range(a, b)]
    assert got == list(range(n))
    for first, last, base, held, (a, b) in sched:
        assert a == base + (0 if first else 3) and b == base + held - (0 if last else 3) and 1 <= held <= 25
    assert sum(1 for c in sched if c[0]) == 1 and sched[0][0] and sched[-1][1] and sum(1 for c in sched if c[1]) == 1
    # the host restatement of the whole clip follows the same calls (a generator that is never asked: no holes)
    color = np.random.default_rng(n).integers(0, 256, (n, 8, 16, 3), dtype=np.uint8)
    out, ref_calls = R.run_clip(color, np.zeros((0, 8, 16, 3), dtype=np.uint8), 24.0, None, orc, model_size=(8, 8))
    assert ref_calls == calls and np.array_equal(out, color)


def test_schedule_refuses_zero_frames():
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    with pytest.raises(ValueError):
        sci.chunk_schedule(0)


# ---- the command line -------------------------------------------------------------------------------------------------------------

def test_cli_parses_the_reference_flags_and_its_own():
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    a = sci.build_parser().parse_args(["--sbs_color_video", "a.mkv", "--sbs_mask_video", "b.mkv"])
    assert (a.max_frames, a.num_inference_steps, a.generator, a.batch, a.video_decoder, a.video_encoder) == (-1, 5, "stereocrafter", 8, "host", "host")
    a = sci.build_parser().parse_args(["--sbs_color_video", "a.txt", "--sbs_mask_video", "b.txt", "--max_frames", "7", "--num_inference_steps", "3",
                                       "--generator", "pkg.mod:fn", "--batch", "4", "--video_decoder", "device", "--video_encoder", "device"])
    assert (a.max_frames, a.num_inference_steps, a.generator, a.batch, a.video_decoder, a.video_encoder) == (7, 3, "pkg.mod:fn", 4, "device", "device")
    with pytest.raises(SystemExit):
        sci.build_parser().parse_args(["--sbs_color_video", "a.mkv"])
    with pytest.raises(SystemExit):
        sci.build_parser().parse_args(["--sbs_color_video", "a.mkv", "--sbs_mask_video", "b.mkv", "--video_encoder", "gpu"])


def test_cli_refusals_leave_no_file_behind(tmp_path, capsys):
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    color, mask = str(tmp_path / "x.npy"), str(tmp_path / "x_mask.npy")
    np.save(color, np.zeros((2, 8, 16, 3), dtype=np.uint8))
    np.save(mask, np.zeros((2, 8, 16, 3), dtype=np.uint8))
    before = sorted(os.listdir(tmp_path))
    base = ["--sbs_color_video", color, "--sbs_mask_video", mask]
    with pytest.raises(SystemExit) as e:                           # the default model is not installed: one clear line
        sci.main(base)
    assert "stereocrafter generator needs StereoCrafter" in str(e.value) and "\n" not in str(e.value)
    for extra, text in ((["--generator", "nocolon"], "pkg.module:callable"), (["--generator", "os.path:nothing_here"], "no callable"),
                        (["--generator", "os.path:join", "--max_frames", "0"], "max_frames")):
        with pytest.raises(SystemExit) as e:
            sci.main(base + extra)
        assert text in str(e.value)
    with pytest.raises(SystemExit) as e:
        sci.main(["--sbs_color_video", str(tmp_path / "missing.mkv"), "--sbs_mask_video", mask, "--generator", "os.path:join"])
    assert "does not exist" in str(e.value)
    with pytest.raises(ValueError):
        sci.main(["--sbs_color_video", str(tmp_path / "list.txt"), "--sbs_mask_video", mask, "--generator", "os.path:join"])
    assert sorted(os.listdir(tmp_path)) == before
    assert sci.load_generator("os.path:join") is os.path.join
