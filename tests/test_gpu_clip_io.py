"""The clip scripts on clip_io: a failure in the middle of a clip leaves neither the `_tmp_` file nor an output behind (3 frames of
two 16 x 16 eyes, batches of 2), and _lib.shared_context hands every caller the context of its own GPU and library variant."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, EW = 3, 16, 16


def _pair(d, ext):
    """A side-by-side colour clip and an infill mask with holes in every frame, as `.mkv` or `.npy` files."""
    from metric_depth_video_toolbox_amd import video_io
    rng = np.random.default_rng(8)
    color = rng.integers(0, 256, (N, H, 2 * EW, 3), dtype=np.uint8)
    mask = np.zeros_like(color)
    mask[:, 4:9, 3:12] = rng.integers(1, 256, (N, 5, 9, 3), dtype=np.uint8)
    mask[:, 6:12, EW + 5:EW + 11] = rng.integers(1, 256, (N, 6, 6, 3), dtype=np.uint8)
    cp, mp = str(d / ("x_stereo" + ext)), str(d / ("x_stereo" + ext + "_infillmask" + ext))
    for path, frames in ((cp, color), (mp, mask)):
        if ext == ".npy":
            np.save(path, frames)
        else:
            with video_io.VideoWriter(path, 2 * EW, H, 25.0) as w:
                for f in frames:
                    w.write(np.ascontiguousarray(f))
    return cp, mp


def _nothing_written(d):
    assert sorted(f for f in os.listdir(d) if "infilled" in f) == [], os.listdir(d)
    assert len(os.listdir(d)) == 2


@pytest.mark.parametrize("ext,codec", [(".mkv", "host"), (".mkv", "device"), (".npy", "host")])
def test_normal_infill_failing_in_its_second_batch_leaves_no_file(tmp_path, monkeypatch, ext, codec):
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni
    cp, mp = _pair(tmp_path, ext)
    real, calls = bni.normal_infill_sbs, []

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("second batch")
        return real(*a, **kw)
    monkeypatch.setattr(bni, "normal_infill_sbs", failing)
    with pytest.raises(RuntimeError, match="second batch"):
        bni.process_pair(cp, mp, batch=2, video_decoder=codec, video_encoder=codec)
    assert len(calls) == 2
    _nothing_written(tmp_path)
    monkeypatch.setattr(bni, "normal_infill_sbs", real)                 # and the same call, left alone, writes the clip
    final = bni.process_pair(cp, mp, batch=2, video_decoder=codec, video_encoder=codec)
    assert final == cp + "_infilled" + ext and sorted(f for f in os.listdir(tmp_path) if "infilled" in f) == [os.path.basename(final)]


@pytest.mark.parametrize("ext,codec", [(".mkv", "host"), (".mkv", "device"), (".npy", "host")])
def test_stereo_crafter_infill_with_a_failing_generator_leaves_no_file(tmp_path, ext, codec):
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    cp, mp = _pair(tmp_path, ext)
    calls = []

    def generate(frames, masks, fps):
        calls.append(tuple(frames.shape))
        raise RuntimeError("the model fell over")
    with pytest.raises(RuntimeError, match="the model fell over"):
        sci.process_pair(cp, mp, generate, batch=2, video_decoder=codec, video_encoder=codec, model_size=(64, 48))
    assert calls == [(N, 48, 64, 3)]
    _nothing_written(tmp_path)


def test_shared_context_is_one_per_device_size_and_library_variant(monkeypatch):
    import torch
    from metric_depth_video_toolbox_amd import _lib, ffv1_device, video_io
    first = _lib.shared_context(0)
    assert _lib.shared_context(0, 16, 16) is first and _lib.shared_context(torch.device("cuda", 0)) is first
    assert _lib.shared_context(0, 32, 16) is not first
    frames = np.random.default_rng(2).integers(0, 256, (2, H, 2 * EW, 3), dtype=np.uint8)
    want = [video_io.encode_frame(f, slices=(4, 4))[0] for f in frames]
    d_frames = torch.from_numpy(frames).cuda()
    assert ffv1_device.encode_frames_on_device(d_frames) == want
    with monkeypatch.context() as m:
        m.setenv("MDVT_LIB_VARIANT", "tuning")
        other = _lib.shared_context(0)
        assert other is not first and _lib.shared_context(0) is other
        assert other._L is _lib.load() and other._L is not first._L           # each calls into the library that made it
        n = C.c_uint64(1 << 63)
        other.call("mdvt_workspace_bytes", C.byref(n))
        assert n.value < 1 << 63
        assert ffv1_device.encode_frames_on_device(d_frames) == want
    assert _lib.shared_context(0) is first and first._L is _lib.load()
    assert ffv1_device.encode_frames_on_device(d_frames) == want


def test_a_device_without_an_index_is_the_current_device():
    import torch
    from metric_depth_video_toolbox_amd import _lib, depth_frames_helper as dfh
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two GPUs to tell the current device from GPU 0; this machine shows {torch.cuda.device_count()}")
    with torch.cuda.device(1):
        assert _lib.device_index(torch.device("cuda")) == 1
        assert _lib.shared_context(torch.device("cuda")).device == 1
        t = torch.arange(4 * 6 * 3, dtype=torch.uint8, device="cuda").reshape(4, 6, 3)
        assert _lib.shared_context(t.device, 6, 4).device == 1
        assert torch.equal(dfh.swap_rb(t), t.flip(-1))
    assert _lib.device_index(torch.device("cuda")) == torch.cuda.current_device()
