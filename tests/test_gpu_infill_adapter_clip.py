"""stereo_crafter_infill.process_pair on .mkv files: 31 frames of 2 x 48 x 32 -- two calls of the chunk schedule and the overlap
between them -- with a deterministic stub generator written in torch, through each decoder and encoder.  The output's frames equal
the host restatement (tests/infill_adapter_ref.py: run_clip with the same stub in NumPy), the frame count and the tmp -> rename
behaviour are right, and a clip without holes never calls the stub."""
import os

import numpy as np
import pytest

import infill_adapter_ref as R

pytestmark = pytest.mark.gpu

EW, H, N, FPS = 48, 32, 31, 25.0
MODEL = (64, 48)                                                    # the model's size in these tests: the host restatement stays quick
CAST = (20, 5, 12)
CALLS = []


def _ramp(T, h, w, xp):
    t, y, x = xp.arange(T).reshape(T, 1, 1), xp.arange(h).reshape(1, h, 1), xp.arange(w).reshape(1, 1, w)
    return [(3 * x + 2 * y + 5 * t) % 256, (x + 4 * y + 40 + 0 * t) % 256, (2 * x + y + 7 * t + 90) % 256]


def stub_numpy(frames, masks, fps):
    """Holes from a fixed ramp, everything else dimmed and colour-cast (so the colour match has work to do): integers only."""
    T, h, w = masks.shape
    ramp = np.stack(np.broadcast_arrays(*_ramp(T, h, w, np)), axis=-1)
    cast = np.clip(frames.astype(np.int64) * 7 // 8 + np.array(CAST), 0, 255)
    return np.where(masks[..., None] != 0, ramp, cast).astype(np.uint8)


def stub_torch(frames, masks, fps):
    import torch
    CALLS.append((tuple(frames.shape), tuple(masks.shape), float(fps)))
    assert frames.is_cuda and frames.dtype == torch.uint8 and masks.is_cuda and masks.dtype == torch.uint8
    T, h, w = masks.shape
    dev = frames.device

    class xp:                                                       # torch.arange on the frames' device, NumPy's spelling
        @staticmethod
        def arange(n):
            return torch.arange(n, device=dev)
    ramp = torch.stack(torch.broadcast_tensors(*_ramp(T, h, w, xp)), dim=-1)
    cast = (torch.div(frames.to(torch.int64) * 7, 8, rounding_mode="floor") + torch.tensor(CAST, device=dev)).clamp(0, 255)
    return torch.where(masks[..., None] != 0, ramp, cast).to(torch.uint8)


def _clip(seed, holes):
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    _, col = SyntheticScene(EW, H, config_id=2, n_fg=4).clip(N)
    sbs = np.ascontiguousarray(np.concatenate([col, col[:, :, ::-1]], axis=2))
    rng = np.random.default_rng(seed)
    mask = R.make_masks(rng, N, H, EW, "mixed") if holes else np.zeros((N, H, 2 * EW, 3), np.uint8)
    if holes:
        mask[4] = 0                                                 # a frame without holes inside a chunk that has some
    return sbs, mask


def _write(path, frames):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoWriter(path, frames.shape[2], frames.shape[1], FPS) as w:
        for f in frames:
            w.write(np.ascontiguousarray(f))


def _read_all(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        return np.stack(list(r)), r.fps


@pytest.fixture(scope="module")
def wanted(orc):
    """The clip with holes and its restatement on the host, computed once."""
    sbs, mask = _clip(11, True)
    want, calls = R.run_clip(sbs, mask, FPS, stub_numpy, orc, model_size=MODEL)
    assert calls == [(True, False, 25), (False, True, 12)] and want.shape == sbs.shape
    assert (want != sbs).any()
    return sbs, mask, want


@pytest.mark.parametrize("decoder,encoder", [("host", "host"), ("device", "device"), ("host", "device")])
def test_clip_equals_the_host_restatement(tmp_path, wanted, decoder, encoder):
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    sbs, mask, want = wanted
    sp, mp = str(tmp_path / "x.mkv_stereo.mkv"), str(tmp_path / "x.mkv_stereo.mkv_infillmask.mkv")
    _write(sp, sbs)
    _write(mp, mask)
    del CALLS[:]
    final = sci.process_pair(sp, mp, stub_torch, batch=7, video_decoder=decoder, video_encoder=encoder, model_size=MODEL)
    assert final == sp + "_infilled.mkv" and os.path.isfile(final) and not os.path.exists(sp + "_tmp_infilled.mkv")
    got, fps = _read_all(final)
    assert got.shape == (N, H, 2 * EW, 3) and abs(fps - FPS) < 1e-6
    bad = np.argwhere((got != want).any(axis=(1, 2, 3))).reshape(-1)
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the restatement"
    # both eyes of both calls asked the stub: 25 frames, then the 6 kept and the 6 new ones
    assert CALLS == [((25, MODEL[1], MODEL[0], 3), (25, MODEL[1], MODEL[0]), FPS)] * 2 + [((12, MODEL[1], MODEL[0], 3), (12, MODEL[1], MODEL[0]), FPS)] * 2
    # max_frames cuts the clip (one call, first and last at once)
    os.remove(final)
    del CALLS[:]
    assert sci.process_pair(sp, mp, stub_torch, 9, video_decoder=decoder, video_encoder=encoder, model_size=MODEL) == final
    short, _ = _read_all(final)
    assert len(short) == 9 and len(CALLS) == 2 and CALLS[0][0][0] == 9


def test_a_clip_without_holes_never_calls_the_stub(tmp_path):
    """Through the command line, at the model's real size: every frame comes back as it went in, and a short mask video is fine."""
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    sbs, mask = _clip(12, False)
    sp, mp = str(tmp_path / "y.mkv_stereo.mkv"), str(tmp_path / "y.mkv_stereo.mkv_infillmask.mkv")
    _write(sp, sbs)
    _write(mp, mask[:5])
    del CALLS[:]
    assert sci.main(["--sbs_color_video", sp, "--sbs_mask_video", mp, "--generator", "test_gpu_infill_adapter_clip:stub_torch",
                     "--video_decoder", "device", "--video_encoder", "device"]) == 0
    final = sp + "_infilled.mkv"
    assert os.path.isfile(final) and not os.path.exists(sp + "_tmp_infilled.mkv")
    got, _ = _read_all(final)
    assert np.array_equal(got, sbs) and not CALLS


def test_a_generator_that_breaks_the_contract_is_refused(tmp_path):
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    sbs, mask = _clip(11, True)
    cn, mn = str(tmp_path / "s.npy"), str(tmp_path / "m.npy")
    np.save(cn, sbs[:3])
    np.save(mn, mask[:3])
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        sci.process_pair(cn, mn, lambda frames, masks, fps: frames.float(), model_size=MODEL)
    assert not os.path.exists(cn + "_infilled.npy")
    assert sci.process_pair(cn, mn, stub_torch, model_size=MODEL) == cn + "_infilled.npy"
    assert np.load(cn + "_infilled.npy").shape == (3, H, 2 * EW, 3)
