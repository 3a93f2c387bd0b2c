"""find_convergence_depth.find end to end on small .mkv files written by the project's writer, with either decoder: the side-car's
text is json.dumps of NumPy's means (tests/convergence_ref.py); and stereo_rerender --find_convergence writes the files of a run
with --convergence_file pointing at that side-car."""
import json
import os

import numpy as np
import pytest

import convergence_ref as cr

pytestmark = pytest.mark.gpu


def _write(path, frames, W, H):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoWriter(path, W, H, 24000 / 1001, bgr=True) as w:
        for f in frames:
            w.write(np.ascontiguousarray(f[..., ::-1]))
    return path


def _clip(d, W, H, N, n_mask, empty=None):
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    dep, col = SyntheticScene(W, H, config_id=3, n_fg=5).clip(N)
    rng = np.random.default_rng(N)
    mask = np.zeros((n_mask, H, W, 3), np.uint8)
    for k in range(n_mask):                                        # a white box that moves, with a soft (grey 240 / 241) rim
        x0, y0 = 5 + 3 * k, 4 + k
        mask[k, y0:y0 + H // 2, x0:x0 + W // 3] = 241
        mask[k, y0 + 2:y0 + H // 2 - 2, x0 + 2:x0 + W // 3 - 2] = 255
        mask[k, y0 - 1] = 240
    if empty is not None:
        mask[empty] = 0
    return (_write(str(d / "v_depth.mkv"), dep, W, H), _write(str(d / "v.mkv"), col, W, H),
            _write(str(d / "v_mask.mkv"), mask, W, H) if n_mask else None, dep, mask)


@pytest.mark.parametrize("decoder", ["host", "device"])
def test_find_writes_numpys_means(tmp_path, decoder, capfd):
    from metric_depth_video_toolbox_amd import find_convergence_depth as fcd
    W, H, N = 160, 90, 11
    dp, _, mp, dep, mask = _clip(tmp_path, W, H, N, 7, empty=2)
    for mask_path, m, max_depth in ((None, None, 100), (mp, mask, 100), (mp, mask, 20)):
        want, n = cr.clip_means(dep, m, max_depth)
        capfd.readouterr()
        got = fcd.find(dp, mask_path, max_depth, batch=4, video_decoder=decoder)
        said = capfd.readouterr().out
        text = open(dp + "_convergence_depths.json").read()
        assert text == json.dumps([float(v) for v in want]), f"mask {mask_path} max_depth {max_depth}"
        assert cr.same_bits(np.array(got, np.float32), want).size == 0 and all(isinstance(v, float) for v in got)
        # the mask video is 4 frames short: said once, and the remaining frames use every pixel
        assert said.count("Failed to read mask video frame") == (1 if m is not None else 0)
        if m is not None:
            assert np.isnan(got[2]) and "NaN" in text and n[7:].tolist() == [W * H] * 4
    assert sorted(os.listdir(tmp_path)) == ["v.mkv", "v_depth.mkv", "v_depth.mkv_convergence_depths.json", "v_mask.mkv"]
    # the CLI: the same file
    os.remove(dp + "_convergence_depths.json")
    assert fcd.main(["--depth_video", dp, "--mask_video", mp, "--max_depth", "20", "--batch", "16", "--video_decoder", decoder]) == 0
    assert open(dp + "_convergence_depths.json").read() == text


def test_find_reads_frame_dumps(tmp_path):
    from metric_depth_video_toolbox_amd import find_convergence_depth as fcd
    rng = np.random.default_rng(3)
    dep = cr.random_depth(rng, 5, 33, 257)
    mask = np.repeat(rng.choice(np.array([0, 255], np.uint8), (5, 33, 257, 1)), 3, axis=3)
    np.save(tmp_path / "d.npy", dep)
    np.save(tmp_path / "m.npy", mask)
    want, _ = cr.clip_means(dep, mask)
    got = fcd.find(str(tmp_path / "d.npy"), str(tmp_path / "m.npy"), batch=2, max_frames=4)
    assert cr.same_bits(np.array(got, np.float32), want[:4]).size == 0 and len(got) == 4


def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("v_depth.mkv_stereo")}


def test_stereo_rerender_find_convergence_equals_the_convergence_file_run(tmp_path):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    W, H, N = 160, 90, 9
    flags = ["--xfov", "50", "--pupillary_distance", "65", "--infill_mask", "--batch", "4"]
    outs = {}
    for how in ("found", "file"):
        d = tmp_path / how
        d.mkdir()
        dp, cp, mp, dep, mask = _clip(d, W, H, N, N, empty=4)
        if how == "found":
            assert sr.main(["--depth_video", dp, "--color_video", cp, "--find_convergence", "--convergence_mask_video", mp] + flags) == 0
            sidecar = open(dp + "_convergence_depths.json").read()
            want, _ = cr.clip_means(dep, mask)
            assert sidecar == json.dumps([float(v) for v in want]) and "NaN" in sidecar
        else:
            (d / "conv.json").write_text(sidecar)
            assert sr.main(["--depth_video", dp, "--color_video", cp, "--convergence_file", str(d / "conv.json")] + flags) == 0
        outs[how] = _outputs(d)
    assert len(outs["file"]) >= 3 and set(outs["found"]) == set(outs["file"])
    for f in outs["file"]:
        assert outs["found"][f] == outs["file"][f], f
    # the curve is not flat: another convergence file gives other renders (the comparison above is not vacuous)
    d = tmp_path / "flat"
    d.mkdir()
    dp, cp, _, _, _ = _clip(d, W, H, N, 0)
    (d / "conv.json").write_text(json.dumps([50.0] * N))
    assert sr.main(["--depth_video", dp, "--color_video", cp, "--convergence_file", str(d / "conv.json")] + flags) == 0
    assert _outputs(d)["v_depth.mkv_stereo.mkv"] != outs["file"]["v_depth.mkv_stereo.mkv"]
