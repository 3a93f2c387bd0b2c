"""A yuv420p colour video end to end: stereo_rerender on a 64 x 48, 5-frame clip whose colour video is YCbCr FFV1 (Golomb-Rice, a
key frame every 3 frames, 2 x 2 slices: what FFmpeg makes of a movie by default, at toy size) writes, with every --video_decoder,
the bytes of the same run on a colour file that holds convert(planes) as RGB."""
import os

import numpy as np
import pytest

import ffv1_ycbcr_ref as yr

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 5


def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("v_depth.mkv_")}


@pytest.fixture(scope="module")
def clip():
    """-> depth frames, the colour planes per frame, convert(planes), the YCbCr packets and their configuration record"""
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    dep, col = SyntheticScene(W, H, config_id=3, n_fg=5).clip(N)
    planes = [(np.ascontiguousarray(f[..., 1]), np.ascontiguousarray(f[::2, ::2, 2]), np.ascontiguousarray(f[::2, ::2, 0])) for f in col]
    p = yr.Params(pix_fmt="yuv420p", coder=0, intra=0, nh=2, nv=2)
    enc = yr.Encoder(p, W, H, gop=3)
    return dep, planes, np.stack([yr.convert(pl, 1, 1) for pl in planes]), [enc.encode(pl) for pl in planes], yr.config_record(p)


def _run(d, clip, colour, decoder):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr, video_io
    dep, planes, rgb, packets, cfg = clip
    d.mkdir()
    dp, cp = str(d / "v_depth.mkv"), str(d / "v.mkv")
    with video_io.VideoWriter(dp, W, H, 24) as w:
        for f in dep:
            w.write(np.ascontiguousarray(f))
    if colour == "rgb":
        with video_io.VideoWriter(cp, W, H, 24) as w:
            for f in rgb:
                w.write(np.ascontiguousarray(f))
    else:
        with open(cp, "wb") as f:
            f.write(yr.mux(packets, W, H, cfg))
    assert sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "45", "--batch", "2", "--infill_mask", "--video_decoder", decoder]) == 0
    return _outputs(d)


def test_a_yuv420p_colour_video_with_every_decoder(tmp_path, clip, capfd, monkeypatch):
    from metric_depth_video_toolbox_amd import ffv1_device
    streamed = []
    collect = ffv1_device.PendingStreamFrames.collect

    def counting_collect(self, *a, **k):
        out = collect(self, *a, **k)
        streamed.append((self.config, len(self.packets) - self.first_out, self.host_frames))
        return out
    monkeypatch.setattr(ffv1_device.PendingStreamFrames, "collect", counting_collect)
    want = _run(tmp_path / "rgb", clip, "rgb", "host")
    assert {"v_depth.mkv_stereo.mkv", "v_depth.mkv_stereo.mkv_infillmask.mkv"} <= set(want)
    capfd.readouterr()
    for decoder in ("host", "device", "device_all"):
        got = _run(tmp_path / decoder, clip, "yuv420p", decoder)
        err = capfd.readouterr().err
        assert set(got) == set(want)
        for f in want:
            assert got[f] == want[f], (decoder, f)
        if decoder == "device":                                        # its one-line notice for a file outside its class
            lines = [ln for ln in err.splitlines() if "color video" in ln]
            assert len(lines) == 1 and "video_decoder device: color video" in lines[0] and "decoded on the host" in lines[0]
            assert not streamed
        else:
            assert "decoded on the host" not in err
    # device_all decoded every colour frame on the GPU itself, batch by batch from the key frame before it
    cfg = clip[4]
    assert sum(n for c, n, h in streamed if c == cfg) == N and all(h == 0 for c, n, h in streamed)
