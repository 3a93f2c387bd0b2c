"""find_convergence_depth's host side -- no GPU: the new entry point's binding, NumPy's float32 summation order restated in plain
Python against NumPy itself (the order csrc/mdvt_convergence.hip reproduces: if a NumPy upgrade changes it, this test says so and
not a GPU test), the command-line flags with their refusals, and the side-car's text."""
import json
import math
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_entry_point_is_exported_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "mdvt_convergence.h")).read()
    declared = sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert declared == sorted(_lib.CONVERGENCE_SYMBOLS) == ["mdvt_convergence_depths"]
    for s in _lib.CONVERGENCE_SYMBOLS:
        assert hasattr(L, s) and s not in _lib.SYMBOLS and s not in _lib.DECODE_SYMBOLS
    main = open(os.path.join(REPO, "include", "mdvt.h")).read()
    assert "mdvt_convergence_depths" not in main
    assert L.mdvt_version() == 15                                   # ABI 0.15: include/mdvt.h is unchanged
    for doc in ("find_convergence_depth.py:53-80", "movie_2_3D.py:408-419"):
        assert doc in hdr


def pw(a):
    """NumPy's pairwise sum of a float32 sequence, every operation rounded to float32."""
    n = len(a)
    if n < 8:
        r = F(0)
        for x in a:
            r = F(r + x)
        return r
    if n <= 128:
        r = [a[k] for k in range(8)]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] = F(r[k] + a[i + k])
            i += 8
        res = F(F(F(r[0] + r[1]) + F(r[2] + r[3])) + F(F(r[4] + r[5]) + F(r[6] + r[7])))
        while i < n:
            res = F(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F(pw(a[:n2]) + pw(a[n2:]))


def chunked_mean(a):
    """The order of a.mean() for a contiguous float32 array: chunks of the ufunc buffer, each summed pairwise, added in sequence."""
    acc = F(0)
    for c in range(0, len(a), 8192):
        acc = F(acc + pw(a[c:c + 8192]))
    return F(acc / F(len(a)))


@pytest.mark.parametrize("n", [1, 7, 8, 117, 128, 130, 8191, 8192, 8193, 8200, 16416, 307200])
def test_numpy_sums_float32_in_chunks_of_8192_pairwise(n):
    assert np.getbufsize() == 8192
    rng = np.random.default_rng(n)
    code = rng.integers(0, 65536, n).astype(np.uint32) << 16
    code[rng.random(n) < 0.05] = 0
    a = code.astype(np.float32) / (255 ** 4 / 100)                  # fcd:60
    assert a.dtype == np.float32
    want = a.mean()
    assert want.dtype == np.float32
    assert chunked_mean(a).tobytes() == want.tobytes()
    if n == 307200:                                                 # a 2-D contiguous array reduces like its flattening
        assert a.reshape(480, 640).mean().tobytes() == want.tobytes()


def test_the_divisor_is_rounded_once_and_the_decode_is_not_the_renders():
    code = (np.arange(65536, dtype=np.uint32) << 16)
    for max_depth in (100, 20, 255):
        ref = code.astype(np.float32) / ((255 ** 4) / max_depth)
        div = np.float32(4228250625.0 / max_depth)
        assert np.array_equal(ref, code.astype(np.float32) / div)
    mult = code.astype(np.float32) * np.float32(100 / 255 ** 4)
    assert (mult != code.astype(np.float32) / np.float32(4228250625.0 / 100)).any()


def test_cli_flags_and_refusals(tmp_path):
    from metric_depth_video_toolbox_amd import clip, find_convergence_depth as fcd, stereo_rerender as sr
    p = fcd.build_parser()
    a = p.parse_args(["--depth_video", "d.mkv"])
    assert (a.mask_video, a.max_depth, a.batch, a.video_decoder) == (None, 100, 64, "host")
    a = p.parse_args(["--depth_video", "d.mkv", "--mask_video", "m.mkv", "--max_depth", "20", "--batch", "8", "--video_decoder", "device"])
    assert (a.mask_video, a.max_depth, a.batch, a.video_decoder) == ("m.mkv", 20, 8, "device")
    with pytest.raises(SystemExit):
        p.parse_args([])
    with pytest.raises(SystemExit):
        p.parse_args(["--depth_video", "d.mkv", "--video_decoder", "gpu"])
    with pytest.raises(FileNotFoundError):
        fcd.find(str(tmp_path / "missing.npy"))
    d = str(tmp_path / "d.npy")
    np.save(d, np.zeros((2, 4, 4, 3), np.uint8))
    with pytest.raises(FileNotFoundError):
        fcd.find(d, str(tmp_path / "missing_mask.npy"))
    with pytest.raises(ValueError, match="video_decoder device"):
        fcd.find(d, video_decoder="device")                         # a frame dump is not decoded
    m = str(tmp_path / "m.npy")
    np.save(m, np.zeros((2, 4, 6, 3), np.uint8))
    with pytest.raises(ValueError, match="same dimensions"):
        fcd.find(d, m)
    assert not os.path.exists(fcd.sidecar_path(d)) and fcd.sidecar_path(d) == d + "_convergence_depths.json"

    ap = sr.build_arg_parser()
    a = ap.parse_args(["--depth_video", d, "--xfov", "45"])
    assert a.find_convergence is False and a.convergence_mask_video is None
    a = ap.parse_args(["--depth_video", d, "--xfov", "45", "--find_convergence", "--convergence_mask_video", m])
    assert a.find_convergence is True and a.convergence_mask_video == m
    c = str(tmp_path / "c.json")
    open(c, "w").write("[1.0, 1.0]")
    with pytest.raises(ValueError, match="--convergence_file"):
        sr.main(["--depth_video", d, "--xfov", "45", "--find_convergence", "--convergence_file", c])
    with pytest.raises(ValueError, match="--find_convergence"):
        sr.main(["--depth_video", d, "--xfov", "45", "--convergence_mask_video", m])
    with pytest.raises(FileNotFoundError):
        sr.main(["--depth_video", d, "--xfov", "45", "--find_convergence", "--convergence_mask_video", str(tmp_path / "no.npy")])
    with pytest.raises(ValueError, match="--convergence_file"):
        clip.run(d, None, xfov=45.0, find_convergence=True, convergence_file=c)
    assert sorted(os.listdir(tmp_path)) == ["c.json", "d.npy", "m.npy"]      # refused before anything was written


def test_the_sidecar_text_is_the_references():
    from metric_depth_video_toolbox_amd import find_convergence_depth as fcd
    vals = [np.float32(1.2345678), float("nan"), np.float32(0.0), np.float32(99.99999)]
    text = fcd.sidecar_text(vals)
    assert text == json.dumps([float(v) for v in vals])             # fcd:78, 94: a bare list of Python floats
    assert text == "[1.2345677614212036, NaN, 0.0, 99.99999237060547]"
    back = json.loads(text)
    assert math.isnan(back[1]) and np.float32(back[0]) == vals[0]
