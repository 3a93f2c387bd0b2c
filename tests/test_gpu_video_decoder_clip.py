"""--video_decoder device end to end: every output of the stereo_rerender CLI is byte-identical to the host decoder's run (with
either encoder, and with an input the device does not decode), and the two-step chain stereo_rerender -> basic_nomal_infill
runs on .mkv files with either decoder."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _inputs(d, W, H, N, config_id=3):
    from metric_depth_video_toolbox_amd import video_io
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    dep, col = SyntheticScene(W, H, config_id=config_id, n_fg=5).clip(N)
    dp, cp = str(d / "v_depth.mkv"), str(d / "v.mkv")
    for path, frames in ((dp, dep), (cp, col)):
        with video_io.VideoWriter(path, W, H, 24000 / 1001, bgr=True) as w:
            for f in frames:
                w.write(np.ascontiguousarray(f[..., ::-1]))
    return dp, cp, dep, col


def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("v_depth.mkv_")}


@pytest.fixture()
def decoded(monkeypatch):
    """Every device-decoded batch of the run: (frames, frames the host had to decode instead)."""
    from metric_depth_video_toolbox_amd import ffv1_device
    seen = []
    collect = ffv1_device.PendingFrames.collect

    def counting_collect(self, *a, **k):
        out = collect(self, *a, **k)
        seen.append((len(self.packets), self.host_frames))
        return out
    monkeypatch.setattr(ffv1_device.PendingFrames, "collect", counting_collect)
    return seen


def _flags(tmp_path, variant, N):
    flags = ["--xfov", "50", "--pupillary_distance", "65", "--create_sbs_depth_video", "--batch", "4"]
    if variant == "points":
        return flags + ["--render_as_pointcloud"]
    (tmp_path / "conv.json").write_text(json.dumps([2.5 + 0.02 * k if k % 5 else float("nan") for k in range(N)]))
    return flags + ["--infill_mask", "--convergence_file", str(tmp_path / "conv.json")]


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("variant", ["product_default", "points"])
def test_device_decoder_gives_the_host_decoders_files(tmp_path, variant, encoder, decoded):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    W, H, N = 160, 90, 11
    flags = _flags(tmp_path, variant, N)
    outs = {}
    for dec in ("host", "device"):
        d = tmp_path / dec
        d.mkdir()
        dp, cp, _, _ = _inputs(d, W, H, N)
        assert sr.main(["--depth_video", dp, "--color_video", cp, "--video_decoder", dec, "--video_encoder", encoder] + flags) == 0
        outs[dec] = _outputs(d)
    want = {"v_depth.mkv_stereo.mkv", "v_depth.mkv_stereo.mkv_holemask.mkv", "v_depth.mkv_stereo.mkv_depth.mkv"}
    if variant == "product_default":
        want.add("v_depth.mkv_stereo.mkv_infillmask.mkv")
    # the device run decoded every frame of both inputs itself
    assert sum(n for n, _ in decoded) == 2 * N and all(h == 0 for _, h in decoded)
    assert set(outs["host"]) == want and set(outs["device"]) == want
    for f in want:
        assert outs["device"][f] == outs["host"][f], f


def test_one_video_for_depth_and_colour(tmp_path, decoded):
    """No --color_video (sr:508-509): the one video is decoded once, on the device."""
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    W, H, N = 96, 54, 6
    outs = {}
    for dec in ("host", "device"):
        d = tmp_path / dec
        d.mkdir()
        dp, _, _, _ = _inputs(d, W, H, N)
        assert sr.main(["--depth_video", dp, "--xfov", "45", "--batch", "4", "--video_decoder", dec]) == 0
        outs[dec] = _outputs(d)
    assert sum(n for n, _ in decoded) == N and all(h == 0 for _, h in decoded)
    assert outs["host"] and outs["device"] == outs["host"]


def test_an_inter_coded_golomb_rice_input_falls_back_to_the_host(tmp_path, decoded, capfd):
    """What FFmpeg writes by default (Golomb-Rice, a key frame every 12): outside the device's class.  The run says so on stderr,
    reads that input on the host, decodes the other on the device, and writes the same bytes."""
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    from oracle import ffv1_ref as ref
    W, H, N = 64, 36, 5
    outs = {}
    for dec in ("host", "device"):
        d = tmp_path / dec
        d.mkdir()
        dp, cp, dep, col = _inputs(d, W, H, N)
        p = ref.Params(coder=0, intra=0, nh=2, nv=2)
        enc = ref.StreamEncoder(p, W, H, gop=3)
        with open(cp, "wb") as f:
            f.write(ref.mux_matroska([enc.encode(np.ascontiguousarray(x)) for x in col], W, H, 24, ref.config_record(p)))
        capfd.readouterr()
        assert sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "45", "--batch", "2", "--video_decoder", dec]) == 0
        err = capfd.readouterr().err
        if dec == "device":
            assert "color video" in err and "decoded on the host" in err and "coder_type" in err
            assert "depth video" not in err
        else:
            assert "decoded on the host" not in err
        outs[dec] = _outputs(d)
    assert sum(n for n, _ in decoded) == N and all(h == 0 for _, h in decoded)       # the depth video went through the device
    assert outs["host"] and outs["device"] == outs["host"]


def test_npy_inputs_refuse_the_device_decoder(tmp_path):
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, stereo_rerender as sr
    a = np.zeros((2, 8, 16, 3), np.uint8)
    dp = str(tmp_path / "d.npy")
    np.save(dp, a)
    with pytest.raises(ValueError, match="video_decoder"):
        sr.main(["--depth_video", dp, "--xfov", "45", "--video_decoder", "device"])
    assert sorted(os.listdir(tmp_path)) == ["d.npy"]                                # refused before anything was read or written
    with pytest.raises(ValueError, match="video_decoder"):
        bni.process_pair(dp, dp, video_decoder="device")
    with pytest.raises(ValueError, match="video_encoder"):
        bni.process_pair(dp, dp, video_encoder="device")


def _read_all(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        return np.stack(list(r)), r.fps


@pytest.mark.parametrize("codec", ["host", "device"])
def test_two_step_chain_on_mkv_files(tmp_path, codec, decoded):
    """stereo_rerender --infill_mask -> basic_nomal_infill on its .mkv outputs: `<sbs_color>_infilled.mkv` holds normal_infill_sbs
    of the decoded inputs frame for frame, equals what the .npy route gives for the same frames, and the tmp file is gone."""
    import torch
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, stereo_rerender as sr
    W, H, N = 160, 90, 9
    dp, cp, _, _ = _inputs(tmp_path, W, H, N)
    assert sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "50", "--infill_mask", "--batch", "4", "--video_decoder", codec,
                    "--video_encoder", codec]) == 0
    sbs_path, mask_path = dp + "_stereo.mkv", dp + "_stereo.mkv_infillmask.mkv"
    del decoded[:]
    assert bni.main(["--sbs_color_video", sbs_path, "--sbs_mask_video", mask_path, "--batch", "4", "--video_decoder", codec,
                     "--video_encoder", codec]) == 0
    final = sbs_path + "_infilled.mkv"
    assert os.path.isfile(final) and not os.path.exists(sbs_path + "_tmp_infilled.mkv") and not os.path.exists(sbs_path + "_infilled.npy")
    if codec == "device":
        assert sum(n for n, _ in decoded) == 2 * N and all(h == 0 for _, h in decoded)
    else:
        assert not decoded
    sbs, fps = _read_all(sbs_path)
    mask, _ = _read_all(mask_path)
    got, got_fps = _read_all(final)
    assert got.shape == (N, H, 2 * W, 3) and abs(got_fps - fps) < 1e-6 and abs(fps - 24000 / 1001) < 1e-3
    want = bni.normal_infill_sbs(torch.from_numpy(sbs).cuda(), torch.from_numpy(mask).cuda()).cpu().numpy()
    assert np.array_equal(got, want)
    assert (want != sbs).any()                                                      # the infill did something
    # the .npy route on the same frames
    cn, mn = str(tmp_path / "s.npy"), str(tmp_path / "m.npy")
    np.save(cn, sbs); np.save(mn, mask)
    assert bni.process_pair(cn, mn) == cn + "_infilled.npy"
    assert np.array_equal(np.load(cn + "_infilled.npy"), got)
    # the other codec setting writes the same file
    other = "host" if codec == "device" else "device"
    first = open(final, "rb").read()
    os.remove(final)
    assert bni.process_pair(sbs_path, mask_path, -1, 3, video_decoder=other, video_encoder=other) == final
    assert open(final, "rb").read() == first


def test_a_short_mask_video_means_no_holes(tmp_path):
    import torch
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, video_io
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    W, H, N, M = 64, 36, 7, 3
    _, col = SyntheticScene(W, H, config_id=2, n_fg=4).clip(N)
    sbs = np.concatenate([col, col[:, :, ::-1]], axis=2)
    rng = np.random.default_rng(4)
    mask = np.zeros((M, H, 2 * W, 3), np.uint8)
    mask[:, 10:20, 30:50] = rng.integers(1, 256, (M, 10, 20, 3), dtype=np.uint8)
    sp, mp = str(tmp_path / "x.mkv_stereo.mkv"), str(tmp_path / "x.mkv_stereo.mkv_infillmask.mkv")
    for path, frames in ((sp, sbs), (mp, mask)):
        with video_io.VideoWriter(path, 2 * W, H, 25.0) as w:
            for f in frames:
                w.write(np.ascontiguousarray(f))
    outs = []
    for dec in ("host", "device"):
        final = bni.process_pair(sp, mp, batch=2, video_decoder=dec)
        assert final == sp + "_infilled.mkv"
        got, _ = _read_all(final)
        outs.append(got)
        os.remove(final)
    full = np.zeros_like(sbs)
    full[:M] = mask
    want = bni.normal_infill_sbs(torch.from_numpy(sbs).cuda(), torch.from_numpy(full).cuda()).cpu().numpy()
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    assert np.array_equal(want[M:], sbs[M:])                                        # no mask frame: nothing to fill
    # max_frames cuts the output
    final = bni.process_pair(sp, mp, 2, video_decoder="device")
    assert _read_all(final)[0].shape[0] == 2
