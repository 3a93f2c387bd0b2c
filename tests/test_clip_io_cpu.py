"""clip_io's shared protocol on the host codec and CPU tensors: ClipOutput's tmp -> final rename and its clean-up after a failure,
ClipInputs closing every reader it opened, fetch against plain indexing, and the module's freedom from torch and the renderer.
Frames are 3 x 16 x 32 x 3 with batches of 2: one full and one partial batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

N, H, W, BATCH = 3, 16, 32, 2


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(3).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def _write_video(path, frames):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoWriter(str(path), frames.shape[2], frames.shape[1], 25.0) as w:
        for f in frames:
            w.write(np.ascontiguousarray(f))
    return str(path)


def _read(path):
    from metric_depth_video_toolbox_amd import video_io
    if path.endswith(".npy"):
        return np.load(path)
    with video_io.VideoReader(path) as r:
        return np.stack(list(r))


def _closed(video_frames):
    return all(not r._h for r in video_frames._readers) and (video_frames._packet_reader is None or not video_frames._packet_reader[0]._h)


@pytest.mark.parametrize("ext", [".npy", ".mkv"])
def test_clip_output_renames_a_complete_file(tmp_path, frames, ext):
    import torch
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    tmp, final = str(tmp_path / ("x_tmp_out" + ext)), str(tmp_path / ("x_out" + ext))
    with ClipOutput(tmp, final, N, (H, W, 3), 25.0 if ext == ".mkv" else None) as out:
        for a in range(0, N, BATCH):
            out.store(torch.from_numpy(frames[a:a + BATCH]), a)
        assert os.path.exists(tmp) and not os.path.exists(final)
    assert sorted(os.listdir(tmp_path)) == ["x_out" + ext]
    assert np.array_equal(_read(final), frames)


@pytest.mark.parametrize("ext", [".npy", ".mkv"])
def test_clip_output_leaves_nothing_after_a_failure(tmp_path, frames, ext):
    import torch
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    tmp, final = str(tmp_path / ("x_tmp_out" + ext)), str(tmp_path / ("x_out" + ext))
    boom = RuntimeError("between two stores")
    with pytest.raises(RuntimeError) as e:
        with ClipOutput(tmp, final, N, (H, W, 3), 25.0 if ext == ".mkv" else None) as out:
            out.store(torch.from_numpy(frames[:BATCH]), 0)
            raise boom
    assert e.value is boom
    assert os.listdir(tmp_path) == []


def test_clip_inputs_closes_every_reader_when_the_block_raises(tmp_path, frames):
    from metric_depth_video_toolbox_amd.clip_io import ClipInputs, VideoFrames
    a, b = _write_video(tmp_path / "a.mkv", frames), _write_video(tmp_path / "b.mkv", frames[:2])
    np.save(tmp_path / "c.npy", frames)
    boom = ValueError("a check after opening")
    with pytest.raises(ValueError) as e:
        with ClipInputs() as inp:
            va = inp.open(a, "a", FileNotFoundError(a))
            vb = inp.open(b, "b", FileNotFoundError(b), run_output=True)
            inp.open(str(tmp_path / "c.npy"), "c", FileNotFoundError("c"))
            assert isinstance(va, VideoFrames) and isinstance(vb, VideoFrames) and not _closed(va) and not _closed(vb)
            assert np.array_equal(va[1], frames[1])
            va.read_packets(0, 1)                                   # the packet reader is one of the readers to close
            raise boom
    assert e.value is boom and _closed(va) and _closed(vb)
    # a file that is not there: the caller's own exception, and what was opened before it is closed too
    mine = Exception("input sbs_mask_video does not exist: nowhere")
    with pytest.raises(Exception) as e:
        with ClipInputs() as inp:
            va = inp.open(a, "a", FileNotFoundError(a))
            inp.open(str(tmp_path / "nowhere.mkv"), "m", mine, run_output=True)
    assert e.value is mine and _closed(va)
    with ClipInputs() as inp:                                       # and the normal exit
        va = inp.open(a, "a", FileNotFoundError(a))
    assert _closed(va)
    os.remove(a)


@pytest.mark.parametrize("kind", ["mkv", "npy", "segments"])
def test_fetch_without_a_device_decoder_is_plain_indexing(tmp_path, frames, kind):
    import torch
    from metric_depth_video_toolbox_amd.clip_io import ClipInputs, SegmentedFrames, fetch, video_parts
    path = str(tmp_path / ("x.npy" if kind == "npy" else "x.mkv"))
    if kind == "npy":
        np.save(path, frames)
    elif kind == "mkv":
        _write_video(path, frames)
    else:                                                           # two video segments, frames [0, 2) and [2, 3), and their index
        segs = [("x.mkv.rank0of2.mkv", 0, 2), ("x.mkv.rank1of2.mkv", 2, 3)]
        for name, lo, hi in segs:
            _write_video(tmp_path / name, frames[lo:hi])
        with open(path + ".index.json", "w") as fh:
            json.dump({"frames": N, "world": 2, "frame_shape": [H, W, 3], "dtype": "uint8",
                       "segments": [{"rank": r, "lo": lo, "hi": hi, "file": name} for r, (name, lo, hi) in enumerate(segs)]}, fh)
    with ClipInputs() as inp:
        f = inp.open(path, "x", FileNotFoundError(path), run_output=kind == "segments")
        inp.on_device(torch.device("cpu"))
        assert inp.ctx is None and inp.dec_ctx is None
        assert len(video_parts(f)) == {"mkv": 1, "npy": 0, "segments": 2}[kind]
        assert isinstance(f, SegmentedFrames) == (kind == "segments")
        for a, b in ((0, 2), (2, 3), (1, 3), (0, 3)):               # the batches of 2, and ranges across the segment boundary
            for got in (inp.fetch(f, a, b), fetch(f, a, b, torch.device("cpu"), None)):
                assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), frames[a:b]), (a, b)
                assert np.array_equal(got.numpy(), np.asarray(f[a:b]))


def test_importing_clip_io_loads_neither_torch_nor_the_renderer():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; import metric_depth_video_toolbox_amd.clip_io as c; "
            "bad = [m for m in ('torch', 'metric_depth_video_toolbox_amd.stereo_rerender', 'metric_depth_video_toolbox_amd.distributed', "
            "'metric_depth_video_toolbox_amd.clip') if m in sys.modules]; "
            "assert not bad, bad; assert c.ClipInputs and c.ClipOutput and c.VideoSink and c.open_output")
    subprocess.run([sys.executable, "-c", code], cwd=repo, check=True)
