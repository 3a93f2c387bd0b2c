"""m2svid_infill.process_pair and stereo_dissoclusion_net_infill.process_pair on tiny .mkv clips written with video_io: 31 frames of
2 x 24 x 16 side by side -- for m2svid one full chunk, the overlap and a remainder -- with a deterministic stub generator for each
engine, written once for NumPy and once for torch.  The outputs equal the NumPy restatement of the whole clip
(tests/infill_engines_ref.py) frame for frame, through the host decoder and encoder once and the device ones once; the frame count
and the tmp -> rename behaviour are right; a short mask video means black masks; a short original or depth video raises."""
import os

import numpy as np
import pytest

import infill_adapter_ref as R
import infill_engines_ref as E

pytestmark = pytest.mark.gpu

EW, H, N, FPS = 24, 16, 31, 25.0
ORG = (20, 14)                                                      # the original video's size (w, h): another one than the eye's
IMAGE, MASK = (16, 12), (6, 4)                                      # the model's sizes in these tests: the host restatement stays quick
CALLS = []


def m2s_stub_numpy(frames, masks, org_frames, fps):
    """Every input shows in every output byte; integers only."""
    T = len(frames)
    s = (masks.reshape(T, -1).astype(np.int64).sum(axis=1) % 7).reshape(T, 1, 1, 1)
    return ((frames.astype(np.int64) * 7 // 8 + org_frames.astype(np.int64) // 4 + s + 11) % 256).astype(np.uint8)


def m2s_stub_torch(frames, masks, org_frames, fps):
    import torch
    CALLS.append((tuple(frames.shape), tuple(masks.shape), tuple(org_frames.shape), float(fps)))
    for t in (frames, masks, org_frames):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    T = len(frames)
    s = (masks.reshape(T, -1).to(torch.int64).sum(dim=1) % 7).reshape(T, 1, 1, 1)
    return ((torch.div(frames.to(torch.int64) * 7, 8, rounding_mode="floor") + torch.div(org_frames.to(torch.int64), 4, rounding_mode="floor")
             + s + 11) % 256).to(torch.uint8)


def sdn_stub_numpy(image, infill_mask, depth):
    d = (depth * np.float32(100)).astype(np.int64)[..., None]
    return ((image.astype(np.int64) * 3 // 4 + infill_mask.astype(np.int64) // 8 + d + 40) % 256).astype(np.uint8)


def sdn_stub_torch(image, infill_mask, depth):
    import torch
    CALLS.append((tuple(image.shape), tuple(infill_mask.shape), tuple(depth.shape)))
    assert image.is_cuda and image.dtype == torch.uint8 and infill_mask.dtype == torch.uint8 and depth.dtype == torch.float32
    assert image.is_contiguous() and infill_mask.is_contiguous() and depth.is_contiguous()
    d = (depth * 100).to(torch.int64)[..., None]
    return ((torch.div(image.to(torch.int64) * 3, 4, rounding_mode="floor") + torch.div(infill_mask.to(torch.int64), 8, rounding_mode="floor")
             + d + 40) % 256).to(torch.uint8)


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
def clip():
    """The clip's four streams: side-by-side colour, infill mask and coded depth, and the original colour video."""
    rng = np.random.default_rng(31)
    sbs = rng.integers(0, 256, (N, H, 2 * EW, 3), dtype=np.uint8)
    sbs[:, :, :, 1] = sbs[:, :, :, 1] // 2 + np.arange(2 * EW, dtype=np.uint8)[None, None, :]      # (some structure besides the noise)
    mask = R.make_masks(rng, N, H, EW, "mixed")
    bg = mask.any(axis=-1) & (rng.random(mask.shape[:3]) < 0.8)
    mask[bg] |= 1                                                   # most hole pixels have no zero channel: they are bg for the finish
    mask[4] = 0                                                     # a frame without holes inside a chunk that has some
    depth = rng.integers(0, 256, (N, H, 2 * EW, 3), dtype=np.uint8)
    org = rng.integers(0, 256, (N + 2, ORG[1], ORG[0], 3), dtype=np.uint8)      # (longer than the clip: the rest is never read)
    return sbs, mask, depth, org


@pytest.fixture(scope="module")
def files(clip, tmp_path_factory):
    d = tmp_path_factory.mktemp("engines_clip")
    sbs, mask, depth, org = clip
    paths = dict(sbs=str(d / "x.mkv_stereo.mkv"), mask=str(d / "x.mkv_stereo.mkv_infillmask.mkv"), depth=str(d / "x.mkv_stereo.mkv_depth.mkv"),
                 org=str(d / "x.mkv"))
    for k, a in (("sbs", sbs), ("mask", mask), ("depth", depth), ("org", org)):
        _write(paths[k], a)
    return paths


@pytest.fixture(scope="module")
def m2s_wanted(clip, orc):
    """The m2svid restatement of the whole clip on the host, pasted and blended, computed once."""
    sbs, mask, _, org = clip
    want = {}
    for blend in (False, True):
        want[blend], calls = E.m2s_run_clip(sbs, mask, org, FPS, m2s_stub_numpy, orc, blend, IMAGE, MASK)
        assert calls == [(True, False, 25), (False, True, 12)] and want[blend].shape == sbs.shape
    assert (want[False] != sbs).any() and (want[True] != want[False]).any()
    return want


@pytest.fixture(scope="module")
def sdn_wanted(clip, orc):
    sbs, mask, depth, _ = clip
    want = E.sdn_run_clip(sbs, mask, depth, sdn_stub_numpy, orc)
    assert (want != sbs).any()
    return want


@pytest.mark.parametrize("decoder,encoder,blend", [("host", "host", False), ("device", "device", True)])
def test_m2svid_clip_equals_the_host_restatement(files, m2s_wanted, decoder, encoder, blend):
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    sp = files["sbs"]
    final, tmp = sp + "_infilled.mkv", sp + "_tmp_infilled.mkv"
    del CALLS[:]
    got_path = m2s.process_pair(sp, files["mask"], files["org"], m2s_stub_torch, batch=7, apply_edge_blending=blend, video_decoder=decoder,
                                video_encoder=encoder, image_size=IMAGE, mask_size=MASK)
    assert got_path == final and os.path.isfile(final) and not os.path.exists(tmp)
    got, fps = _read_all(final)
    os.remove(final)
    assert got.shape == (N, H, 2 * EW, 3) and abs(fps - FPS) < 1e-6
    bad = np.argwhere((got != m2s_wanted[blend]).any(axis=(1, 2, 3))).reshape(-1)
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the restatement"
    # both eyes of both calls asked the stub: 25 frames, then the 6 kept and the 6 new ones
    shapes = lambda T: ((T, IMAGE[1], IMAGE[0], 3), (T, MASK[1], MASK[0]), (T, IMAGE[1], IMAGE[0], 3), FPS)
    assert CALLS == [shapes(25)] * 2 + [shapes(12)] * 2


def test_m2svid_command_line_on_a_clip_without_holes(files, clip, tmp_path):
    """Through the command line, at the model's real sizes: no mask has a hole, so the generator is never asked and every frame comes
    back as it went in (blended too: an alpha of zero everywhere)."""
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    mp = str(tmp_path / "black_mask.mkv")
    _write(mp, np.zeros((3, H, 2 * EW, 3), np.uint8))              # (and it ends early)
    sp = files["sbs"]
    del CALLS[:]
    assert m2s.main(["--color_video", files["org"], "--sbs_color_video", sp, "--sbs_mask_video", mp, "--max_frames", "27", "--apply_edge_blending",
                     "--generator", "test_gpu_infill_engines_clip:m2s_stub_torch", "--video_decoder", "device", "--video_encoder", "device"]) == 0
    final = sp + "_infilled.mkv"
    assert os.path.isfile(final) and not os.path.exists(sp + "_tmp_infilled.mkv")
    got, _ = _read_all(final)
    os.remove(final)
    assert np.array_equal(got, clip[0][:27]) and not CALLS


@pytest.mark.parametrize("decoder,encoder,cli", [("host", "host", False), ("device", "device", True)])
def test_sdn_clip_equals_the_host_restatement(files, sdn_wanted, decoder, encoder, cli):
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    sp = files["sbs"]
    final, tmp = sp + "_infilled.mkv", sp + "_tmp_infilled.mkv"
    del CALLS[:]
    if cli:
        assert sdn.main(["--sbs_color_video", sp, "--sbs_mask_video", files["mask"], "--sbs_depth_video", files["depth"], "--batch", "7",
                         "--generator", "test_gpu_infill_engines_clip:sdn_stub_torch", "--video_decoder", decoder, "--video_encoder", encoder]) == 0
    else:
        assert sdn.process_pair(sp, files["mask"], files["depth"], sdn_stub_torch, batch=7, video_decoder=decoder, video_encoder=encoder) == final
    assert os.path.isfile(final) and not os.path.exists(tmp)
    got, fps = _read_all(final)
    os.remove(final)
    assert got.shape == (N, H, 2 * EW, 3) and abs(fps - FPS) < 1e-6
    bad = np.argwhere((got != sdn_wanted).any(axis=(1, 2, 3))).reshape(-1)
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the restatement"
    # each batch asked the stub once per eye
    batches = [7, 7, 7, 7, 3]
    assert CALLS == [((b, H, EW, 3), (b, H, EW, 3), (b, H, EW)) for b in batches for _ in (0, 1)]


def test_short_mask_videos_give_black_masks(clip, orc, tmp_path):
    """Frame dumps (no codec in the way): a mask clip of 2 frames under 5 colour frames."""
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    sbs, mask, depth, org = clip
    p = {k: str(tmp_path / (k + ".npy")) for k in ("sbs", "mask", "depth", "org")}
    for k, a in (("sbs", sbs[:5]), ("mask", mask[:2]), ("depth", depth[:5]), ("org", org[:5])):
        np.save(p[k], a)
    final = p["sbs"] + "_infilled.npy"
    assert m2s.process_pair(p["sbs"], p["mask"], p["org"], m2s_stub_torch, apply_edge_blending=True, image_size=IMAGE, mask_size=MASK) == final
    want, _ = E.m2s_run_clip(sbs[:5], mask[:2], org[:5], 30.0, m2s_stub_numpy, orc, True, IMAGE, MASK)
    got = np.load(final)
    assert np.array_equal(got, want) and not (got[:2] == sbs[:2]).all()
    os.remove(final)
    assert sdn.process_pair(p["sbs"], p["mask"], p["depth"], sdn_stub_torch, batch=2) == final
    want = E.sdn_run_clip(sbs[:5], mask[:2], depth[:5], sdn_stub_numpy, orc)
    got = np.load(final)
    assert np.array_equal(got, want) and np.array_equal(got[2:], sbs[2:5]) and not np.array_equal(got[:2], sbs[:2])      # black masks: out == img
    assert not os.path.exists(p["sbs"] + "_tmp_infilled.npy")


def test_a_short_original_or_depth_video_raises(clip, tmp_path):
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    sbs, mask, depth, org = clip
    p = {k: str(tmp_path / (k + ".npy")) for k in ("sbs", "mask", "depth", "org")}
    for k, a in (("sbs", sbs[:5]), ("mask", mask[:5]), ("depth", depth[:3]), ("org", org[:4])):
        np.save(p[k], a)
    del CALLS[:]
    with pytest.raises(ValueError, match="org color ended early"):
        m2s.process_pair(p["sbs"], p["mask"], p["org"], m2s_stub_torch, image_size=IMAGE, mask_size=MASK)
    with pytest.raises(ValueError, match="depth video ended early"):
        sdn.process_pair(p["sbs"], p["mask"], p["depth"], sdn_stub_torch)
    assert not CALLS and sorted(os.listdir(tmp_path)) == ["depth.npy", "mask.npy", "org.npy", "sbs.npy"]
    # as many frames as are asked for is enough
    assert m2s.process_pair(p["sbs"], p["mask"], p["org"], m2s_stub_torch, 4, image_size=IMAGE, mask_size=MASK) == p["sbs"] + "_infilled.npy"
    assert len(np.load(p["sbs"] + "_infilled.npy")) == 4
    # a generator that breaks the contract is refused and leaves no file
    os.remove(p["sbs"] + "_infilled.npy")
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        m2s.process_pair(p["sbs"], p["mask"], p["org"], lambda f, m, o, fps: f.float(), 4, image_size=IMAGE, mask_size=MASK)
    assert sorted(os.listdir(tmp_path)) == ["depth.npy", "mask.npy", "org.npy", "sbs.npy"]
