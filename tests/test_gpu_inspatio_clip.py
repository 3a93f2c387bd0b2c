"""tools/inspatio_world_infill.py on tiny clips with a stub generator, byte for byte against tests/inspatio_ref.py's restatement of the
whole step: eyes of 64 x 40, chunks of 10 frames so that 24 frames take more than three calls, host and device codecs, a list, --max_frames,
an eye without holes (the generator is not asked for it), blending on and off, and what the stub was handed, bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import infill_adapter_ref as iar
import inspatio_ref as ir

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EW, H, N, FPS, CHUNK = 64, 40, 24, 25.0, 10
ORG = (50, 30)                                                      # the original video's size (w, h)
MODEL = (52, 30)                                                    # the model's size in these tests
PROMPT = "a test scene"
CALLS, HANDED = [], []


def stub_numpy(source, render, mask, fps, text_prompt):
    """The render moved by (1, -2), and under the holes (mask below 255) bytes made of the source: integers only."""
    moved = np.roll(render, (1, -2), axis=(1, 2)).astype(np.int64)
    fill = (source.astype(np.int64) * 5 // 7 + 13) % 256
    return np.where((mask == 255)[..., None], moved, fill).astype(np.uint8)


def stub_torch(source, render, mask, fps, text_prompt):
    import torch
    for t in (source, render, mask):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    CALLS.append((tuple(source.shape), tuple(render.shape), tuple(mask.shape), float(fps), text_prompt))
    HANDED.append((source.cpu().numpy(), render.cpu().numpy(), mask.cpu().numpy()))
    moved = torch.roll(render, (1, -2), dims=(1, 2)).to(torch.int64)
    fill = (torch.div(source.to(torch.int64) * 5, 7, rounding_mode="floor") + 13) % 256
    return torch.where((mask == 255)[..., None], moved, fill).to(torch.uint8)


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("inspatio_world_infill_tool", os.path.join(REPO, "tools", "inspatio_world_infill.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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
    rng = np.random.default_rng(64)
    sbs = rng.integers(0, 256, (N, H, 2 * EW, 3), dtype=np.uint8)
    mask = iar.make_masks(rng, N, H, EW, "mixed")
    mask[4] = 0                                                     # a frame without holes inside a chunk that has some
    mask[12:, :, :EW] = 0                                           # the left eye of the last call has no hole: the generator is not asked
    org = rng.integers(0, 256, (N + 2, ORG[1], ORG[0], 3), dtype=np.uint8)
    return sbs, mask, org


@pytest.fixture(scope="module")
def files(clip, tmp_path_factory):
    d = tmp_path_factory.mktemp("inspatio_clip")
    sbs, mask, org = clip
    paths = dict(sbs=str(d / "x.mkv_stereo.mkv"), mask=str(d / "x.mkv_stereo.mkv_infillmask.mkv"), org=str(d / "x.mkv"))
    for k, a in (("sbs", sbs), ("mask", mask), ("org", org)):
        _write(paths[k], a)
    return paths


@pytest.fixture(scope="module")
def wanted(clip, orc):
    """The restatement of the whole clip on the host, with and without blending, and what its stub was handed; computed once."""
    sbs, mask, org = clip
    want, handed = {}, {}
    for blend in (False, True):
        seen = []

        def gen(source, render, m, fps, prompt):
            seen.append((source.copy(), render.copy(), m.copy()))
            assert fps == FPS and prompt == PROMPT
            return stub_numpy(source, render, m, fps, prompt)
        want[blend], calls = ir.run_clip(sbs, mask, org, FPS, gen, orc, blend, MODEL, CHUNK, PROMPT)
        handed[blend] = seen
        from metric_depth_video_toolbox_amd import inspatio_world as iw
        assert calls == [(f, l, held) for f, l, _, held, _ in iw.chunk_schedule(N, CHUNK)] and len(calls) >= 3 and want[blend].shape == sbs.shape
    assert (want[False] != sbs).any() and (want[True] != want[False]).any()
    assert 3 <= len(handed[True]) < 2 * len(calls), "an eye of some call has no hole: the generator is not asked for it"
    assert {len(h[0]) for h in handed[True]} <= {9, 21}, "the frame counts are padded to 4 k - 3 with k a multiple of 3"
    return want, handed


@pytest.mark.parametrize("decoder,encoder,blend", [("host", "host", False), ("device", "device", True)])
def test_the_clip_equals_the_host_restatement(tool, files, wanted, decoder, encoder, blend):
    want, handed = wanted
    sp = files["sbs"]
    final, tmp = sp + "_infilled.mkv", sp + "_tmp_infilled.mkv"
    del CALLS[:], HANDED[:]
    got_path = tool.process_pair(sp, files["mask"], files["org"], stub_torch, batch=7, apply_edge_blending=blend, text_prompt=PROMPT,
                                 video_decoder=decoder, video_encoder=encoder, model_size=MODEL, chunk=CHUNK)
    assert got_path == final and os.path.isfile(final) and not os.path.exists(tmp)
    got, fps = _read_all(final)
    os.remove(final)
    assert got.shape == (N, H, 2 * EW, 3) and abs(fps - FPS) < 1e-6
    bad = np.argwhere((got != want[blend]).any(axis=(1, 2, 3))).reshape(-1)
    assert len(bad) == 0, f"frames {bad.tolist()} differ from the restatement"
    assert CALLS == [(h[0].shape, h[1].shape, h[2].shape, FPS, PROMPT) for h in handed[blend]]
    for mine, theirs in zip(HANDED, handed[blend]):                 # what the stub was handed, bit for bit
        for a, b in zip(mine, theirs):
            assert np.array_equal(a, b)


def test_the_command_line_with_a_list_and_max_frames(tool, files, clip, orc, tmp_path):
    sbs, mask, org = clip
    lists = {k: str(tmp_path / (k + ".txt")) for k in ("sbs", "mask", "org")}
    for k in lists:
        with open(lists[k], "w") as f:
            f.write("# one clip\n" + files[k] + "\n")
    del CALLS[:], HANDED[:]
    assert tool.main(["--color_video", lists["org"], "--sbs_color_video", lists["sbs"], "--sbs_mask_video", lists["mask"], "--max_frames", "13",
                      "--apply_edge_blending", "--text_prompt", PROMPT, "--chunk", str(CHUNK), "--generator", "test_gpu_inspatio_clip:stub_torch",
                      "--video_decoder", "device", "--video_encoder", "device"]) == 0
    final = files["sbs"] + "_infilled.mkv"
    assert os.path.isfile(final) and not os.path.exists(files["sbs"] + "_tmp_infilled.mkv")
    got, _ = _read_all(final)
    os.remove(final)
    # the command line runs at the model's real size
    want, calls = ir.run_clip(sbs[:13], mask[:13], org, FPS, stub_numpy, orc, True, (832, 480), CHUNK, PROMPT)
    assert calls == [(True, False, 10), (False, True, 9)] and np.array_equal(got, want)
    assert [c[0] for c in CALLS] == [(21, 480, 832, 3)] * 2 + [(9, 480, 832, 3)] * 2


def test_a_clip_without_holes_never_asks_the_generator(tool, files, clip, tmp_path):
    mp = str(tmp_path / "black_mask.mkv")
    _write(mp, np.zeros((3, H, 2 * EW, 3), np.uint8))              # (and it ends early: black masks for the rest)
    del CALLS[:], HANDED[:]
    final = tool.process_pair(files["sbs"], mp, files["org"], stub_torch, 17, apply_edge_blending=True, model_size=MODEL, chunk=CHUNK)
    got, _ = _read_all(final)
    os.remove(final)
    assert np.array_equal(got, clip[0][:17]) and not CALLS


def test_a_short_colour_video_and_a_broken_generator_leave_no_file(tool, clip, tmp_path):
    sbs, mask, org = clip
    p = {k: str(tmp_path / (k + ".npy")) for k in ("sbs", "mask", "org")}
    for k, a in (("sbs", sbs[:5]), ("mask", mask[:5]), ("org", org[:4])):
        np.save(p[k], a)
    del CALLS[:], HANDED[:]
    with pytest.raises(ValueError, match="Original color video ended before SBS video"):
        tool.process_pair(p["sbs"], p["mask"], p["org"], stub_torch, model_size=MODEL, chunk=CHUNK)
    assert not CALLS and sorted(os.listdir(tmp_path)) == ["mask.npy", "org.npy", "sbs.npy"]
    assert tool.process_pair(p["sbs"], p["mask"], p["org"], stub_torch, 4, model_size=MODEL, chunk=CHUNK) == p["sbs"] + "_infilled.npy"
    assert len(np.load(p["sbs"] + "_infilled.npy")) == 4
    os.remove(p["sbs"] + "_infilled.npy")
    with pytest.raises(TypeError, match="uint8 CUDA tensor"):
        tool.process_pair(p["sbs"], p["mask"], p["org"], lambda s, r, m, fps, t: r[:3], 4, model_size=MODEL, chunk=CHUNK)
    assert sorted(os.listdir(tmp_path)) == ["mask.npy", "org.npy", "sbs.npy"]
