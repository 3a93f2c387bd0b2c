"""step_clip.StepClip's device phase on a 64 x 36 colour clip of 3 frames, once as a .npy dump and once as an .mkv with the device
decoder and encoder: exactly one context per clip on both routes, closed after a normal exit and after an exception raised inside the
block; the final file with its 3 frames after the one, neither tmp nor final file after the other.  The loop body copies the frames
through; the exception is a RuntimeError of the body's own, on the host."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, W, H = 3, 64, 36


def _read(path):
    from metric_depth_video_toolbox_amd import video_io
    if path.endswith(".npy"):
        return np.load(path)
    with video_io.VideoReader(path) as r:
        frames = np.empty((r.frames, r.height, r.width, 3), np.uint8)
        for k in range(r.frames):
            assert r.read_into(frames[k])
        return frames


@pytest.fixture(scope="module")
def color():
    return np.random.default_rng(21).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


@pytest.fixture
def contexts(monkeypatch):
    """_lib.Context counted: (the contexts made, the ones closed while open)."""
    from metric_depth_video_toolbox_amd import _lib
    made, closed = [], []

    class Counted(_lib.Context):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def close(self):
            if getattr(self, "_h", None) is not None and self._h.value:
                closed.append(self)
            super().close()
    monkeypatch.setattr(_lib, "Context", Counted)
    return made, closed


@pytest.mark.parametrize("route", ["npy", "mkv_device_codecs"])
def test_one_context_per_clip_closed_either_way_and_the_files_that_stay(tmp_path, color, contexts, route):
    from metric_depth_video_toolbox_amd import step_clip, video_io
    made, closed = contexts
    if route == "npy":
        path, codecs = str(tmp_path / "x.npy"), ("host", "host")
        np.save(path, color)
    else:
        path, codecs = str(tmp_path / "x.mkv"), ("device", "device")
        with video_io.VideoWriter(path, W, H, 24.0) as wr:
            for f in color:
                wr.write(f)
    tmp, final = step_clip.output_pair(path, route != "npy")

    def run(fail_at=None):
        with step_clip.StepClip() as clip:
            frames, = clip.open_checked([(path, "color_video", Exception("missing"))], *codecs, lambda n: n)
            assert (clip.n, clip.H, clip.W) == (N, H, W) and not made
            # (the file states a frame's duration in whole nanoseconds: 24 frames per second come back as 23.9999998)
            assert clip.fps is None if route == "npy" else abs(clip.fps - 24.0) < 1e-6
            with clip.device(tmp, final) as (ctx, fetch, store):
                assert made == [ctx] and not closed
                for a in range(N):
                    if a == fail_at:
                        raise RuntimeError("the loop body failed")
                    store(fetch(frames, a, a + 1), a)
                    assert os.path.exists(tmp) and not os.path.exists(final)
            assert os.path.exists(final) and not os.path.exists(tmp) and not closed     # renamed at the block's end; the context lives on
    # an exception from inside the block, after two frames were stored
    with pytest.raises(RuntimeError, match="the loop body failed"):
        run(fail_at=2)
    assert len(made) == 1 and closed == made
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(path)]                     # neither tmp nor final
    # the normal exit
    del made[:], closed[:]
    run()
    assert len(made) == 1 and closed == made
    assert sorted(os.listdir(tmp_path)) == sorted([os.path.basename(path), os.path.basename(final)])
    got = _read(final)
    assert got.shape == (N, H, W, 3) and np.array_equal(got, color)
