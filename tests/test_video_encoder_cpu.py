"""--video_encoder / clip.run(video_encoder=) / ffv1_device argument checks -- no GPU."""
import os

import numpy as np
import pytest


def test_cli_flag_parses_with_host_default():
    from metric_depth_video_toolbox_amd.stereo_rerender import build_arg_parser
    ap = build_arg_parser()
    base = ["--depth_video", "d.mkv", "--xfov", "45"]
    assert ap.parse_args(base).video_encoder == "host"
    assert ap.parse_args(base + ["--video_encoder", "device"]).video_encoder == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--video_encoder", "gpu"])


def test_cli_refuses_device_encoder_with_npy_before_reading(tmp_path, monkeypatch):
    from metric_depth_video_toolbox_amd import clip, stereo_rerender
    depth = tmp_path / "d.npy"
    np.save(depth, np.zeros((2, 8, 8, 3), np.uint8))

    def no_run(*a, **k):
        raise AssertionError("clip.run must not be reached")
    monkeypatch.setattr(clip, "run", no_run)
    with pytest.raises(ValueError, match="--video_encoder device encodes .mkv outputs"):
        stereo_rerender.main(["--depth_video", str(depth), "--xfov", "45", "--video_encoder", "device"])


def test_cli_passes_the_device_encoder_on(tmp_path, monkeypatch):
    from metric_depth_video_toolbox_amd import clip, stereo_rerender, video_io
    depth = tmp_path / "d.mkv"
    with video_io.VideoWriter(str(depth), 8, 8, 30.0) as w:
        w.write(np.zeros((8, 8, 3), np.uint8))
    seen = {}

    class Stop(Exception):
        pass

    def fake_run(*a, **k):
        seen.update(k)
        raise Stop()
    monkeypatch.setattr(clip, "run", fake_run)
    with pytest.raises(Stop):
        stereo_rerender.main(["--depth_video", str(depth), "--xfov", "45", "--video_encoder", "device"])
    assert seen["video_encoder"] == "device"
    seen.clear()
    with pytest.raises(Stop):
        stereo_rerender.main(["--depth_video", str(depth), "--xfov", "45"])
    assert seen["video_encoder"] == "host"


def test_clip_run_refuses_before_opening_anything(tmp_path):
    from metric_depth_video_toolbox_amd import clip
    missing = str(tmp_path / "never_read.npy")
    with pytest.raises(ValueError, match="not encoded"):
        clip.run(missing, None, video_encoder="device", xfov=45.0)
    with pytest.raises(ValueError, match="video_encoder must be one of"):
        clip.run(missing, None, video_encoder="cuda", xfov=45.0)
    assert not os.path.exists(missing)


def test_video_sink_refuses_unknown_encoder(tmp_path):
    from metric_depth_video_toolbox_amd import clip
    with pytest.raises(ValueError, match="encoder must be one of"):
        clip.VideoSink(str(tmp_path / "x.mkv"), 8, 8, 30.0, encoder="gpu")
    s = clip.VideoSink(str(tmp_path / "y.mkv"), 8, 8, 30.0, encoder="device")
    assert s.device
    s.write_from(np.zeros((1, 8, 8, 3), np.uint8), 0, 1)       # the host path stays available in device mode
    assert s.close() == 1


def test_python_argument_checks():
    import torch
    from metric_depth_video_toolbox_amd import ffv1_device
    with pytest.raises(ValueError, match="torch.Tensor"):
        ffv1_device.encode_frames_on_device(np.zeros((1, 4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ffv1_device.encode_frames_on_device(torch.zeros((1, 4, 4, 3), dtype=torch.float32))
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\) or \(N, H, W\)"):
        ffv1_device.encode_frames_on_device(torch.zeros((1, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA device"):
        ffv1_device.encode_frames_on_device(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    # slice counts the host encoder refuses (a CPU tensor dressed as a CUDA one: no device needed)
    for shape, sl in (((1, 4, 4, 3), (0, 1)), ((1, 4, 4, 3), (1, 0)), ((1, 4, 4, 3), (5, 1)), ((1, 4, 4), (1, 5)),
                      ((1, 40, 40, 3), (33, 32))):
        with pytest.raises(ValueError, match="slices"):
            ffv1_device.check_frames(_as_cuda(torch.zeros(shape, dtype=torch.uint8)), sl)
    assert ffv1_device.check_frames(_as_cuda(torch.zeros((2, 4, 6), dtype=torch.uint8)), (6, 4)) == (2, 4, 6, 1)


def _as_cuda(t):
    import torch

    class T(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    return t.as_subclass(T)
