"""--video_decoder device_all end to end: inputs of the class FFmpeg and OpenCV write by default (Golomb-Rice, inter frames) are
decoded on the device by the clip scripts, every output byte-identical to the host decoder's run; the device decoded every frame
itself (counted), and nothing about the host appears on stderr."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N = 64, 36, 5


def _golomb_file(path, frames, gop=3, slices=(2, 2)):
    from oracle import ffv1_ref as ref
    h, w = frames[0].shape[:2]
    p = ref.Params(coder=0, intra=0, nh=slices[0], nv=slices[1])
    enc = ref.StreamEncoder(p, w, h, gop=gop)
    with open(path, "wb") as f:
        f.write(ref.mux_matroska([enc.encode(np.ascontiguousarray(x)) for x in frames], w, h, 24, ref.config_record(p)))


def _inputs(d, depth_class="golomb", color_class="golomb"):
    from metric_depth_video_toolbox_amd import video_io
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    dep, col = SyntheticScene(W, H, config_id=3, n_fg=5).clip(N)
    dp, cp = str(d / "v_depth.mkv"), str(d / "v.mkv")
    for path, frames, cls in ((dp, dep, depth_class), (cp, col, color_class)):
        if cls == "golomb":
            _golomb_file(path, frames)
        else:
            with video_io.VideoWriter(path, W, H, 24) as w:
                for f in frames:
                    w.write(np.ascontiguousarray(f))
    return dp, cp


def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("v_depth.mkv_")}


@pytest.fixture()
def decoded(monkeypatch):
    """Every device-decoded batch of the run: (call, frames stored, frames the host had to decode instead)."""
    from metric_depth_video_toolbox_amd import ffv1_device
    seen = []
    for cls, name in ((ffv1_device.PendingFrames, "frames"), (ffv1_device.PendingStreamFrames, "stream")):
        def counting_collect(self, *a, _collect=cls.collect, _name=name, **k):
            out = _collect(self, *a, **k)
            seen.append((_name, len(self.packets) - getattr(self, "first_out", 0), self.host_frames))
            return out
        monkeypatch.setattr(cls, "collect", counting_collect)
    return seen


def _rerender_both(tmp_path, capfd, **classes):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    outs, errs = {}, {}
    for dec in ("host", "device_all"):
        d = tmp_path / dec
        d.mkdir()
        dp, cp = _inputs(d, **classes)
        capfd.readouterr()
        assert sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "45", "--infill_mask", "--batch", "2", "--video_decoder", dec]) == 0
        errs[dec] = capfd.readouterr().err
        outs[dec] = _outputs(d)
    assert outs["host"] and outs["device_all"] == outs["host"]
    assert "decoded on the host" not in errs["device_all"] and "decoded on the host" not in errs["host"]
    return outs


def test_stereo_rerender_on_two_golomb_rice_inputs(tmp_path, capfd, decoded):
    _rerender_both(tmp_path, capfd)
    assert all(kind == "stream" and h == 0 for kind, _, h in decoded)
    assert sum(n for _, n, _ in decoded) == 2 * N                       # the device decoded every frame of both inputs


def test_stereo_rerender_on_one_file_of_each_class(tmp_path, capfd, decoded):
    _rerender_both(tmp_path, capfd, depth_class="range")
    assert all(h == 0 for _, _, h in decoded)
    assert sum(n for kind, n, _ in decoded if kind == "frames") == N and sum(n for kind, n, _ in decoded if kind == "stream") == N


def _reencode(src, dst, gop=3):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(src) as r:
        with video_io.VideoWriter(dst, r.width, r.height, r.fps, slices=(2, 2), coder=0, gop=gop) as w:
            for f in r:
                w.write(f)


def _infill_both(tmp_path, capfd, monkeypatch=None, bound=None):
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, clip_io, stereo_rerender as sr
    dp, cp = _inputs(tmp_path, "range", "range")
    assert sr.main(["--depth_video", dp, "--color_video", cp, "--xfov", "45", "--infill_mask", "--batch", "4"]) == 0
    sbs, mask = str(tmp_path / "g.mkv_stereo.mkv"), str(tmp_path / "g.mkv_stereo.mkv_infillmask.mkv")
    _reencode(dp + "_stereo.mkv", sbs)
    _reencode(dp + "_stereo.mkv_infillmask.mkv", mask)
    if bound is not None:
        monkeypatch.setattr(clip_io, "KEY_SCAN_FRAMES", bound)
    got, errs = {}, {}
    for dec in ("host", "device_all"):
        capfd.readouterr()
        final = bni.process_pair(sbs, mask, batch=2, video_decoder=dec)
        errs[dec] = capfd.readouterr().err
        got[dec] = open(final, "rb").read()
        os.remove(final)
    assert got["device_all"] == got["host"]
    return errs


def test_basic_nomal_infill_on_outputs_in_the_new_class(tmp_path, capfd, decoded):
    errs = _infill_both(tmp_path, capfd)
    assert "decoded on the host" not in errs["device_all"]
    assert all(kind == "stream" and h == 0 for kind, _, h in decoded) and sum(n for _, n, _ in decoded) == 2 * N


def test_key_frames_further_apart_than_the_bound_fall_back(tmp_path, capfd, monkeypatch, decoded):
    """gop 3 against a bound of 1 frame: the batch at frame 2 finds no key frame; each file says so once and is read on the host."""
    errs = _infill_both(tmp_path, capfd, monkeypatch, bound=1)
    err = errs["device_all"]
    assert err.count("decoded on the host") == 2 and err.count("key-frame distance") == 2 and "intra" in err
    assert "sbs" in err.lower() and "mask" in err.lower()
    assert all(h == 0 for _, _, h in decoded) and sum(n for _, n, _ in decoded) < 2 * N
