"""tools/scene_detect.py and tools/movie_2_3D.py on small clips: the scene CSV equals tests/scene_ref.py's text byte for byte with
every decoder, batch size and detector; the driver's scene clips decode to the movie's frame ranges; the whole pipeline with stub
generators writes every file the reference's plan names, joins them, and a rerun resumes."""
import importlib.util
import os

import numpy as np
import pytest

import scene_ref as sr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS = 24.0


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool("scene_detect")


@pytest.fixture(scope="module")
def movie(tmp_path_factory):
    """40 frames of 48 x 32, three shots with cuts in front of frames 16 and 32 -> (path of the .mkv, path of the .npy, frames)."""
    from metric_depth_video_toolbox_amd import video_io
    d = tmp_path_factory.mktemp("scene_clip")
    frames = sr.three_shot_clip()
    mkv, npy = str(d / "movie.mkv"), str(d / "movie.npy")
    with video_io.VideoWriter(mkv, 48, 32, FPS) as w:
        for f in frames:
            w.write(f)
    np.save(npy, frames)
    want = {det: sr.clip_csv(frames, FPS, det) for det in ("content", "adaptive")}
    assert all(text.count("\n") == 5 and text.startswith("Timecode List:,00:00:00.667,00:00:01.333\n") for text in want.values()), want
    return mkv, npy, frames, want


def _read(path):
    with open(path, newline="") as fh:
        return fh.read()


@pytest.mark.parametrize("detector", ["content", "adaptive"])
def test_csv_equals_the_restatement_with_every_decoder_and_batch(tool, movie, tmp_path, detector):
    mkv, npy, frames, want = movie
    for k, extra in enumerate((["--video_decoder", "host"], ["--video_decoder", "device"], ["--video_decoder", "device_all"],
                               ["--batch", "7"], ["--batch", "1"], ["--batch", "7", "--video_decoder", "device"])):
        out = str(tmp_path / f"{detector}{k}-Scenes.csv")
        assert tool.main(["--color_video", mkv, "--detector", detector, "--output", out] + extra) == 0
        assert _read(out) == want[detector], extra
    out = str(tmp_path / "dump-Scenes.csv")
    assert tool.main(["--color_video", npy, "--detector", detector, "--fps", str(FPS), "--batch", "9", "--output", out]) == 0
    assert _read(out) == want[detector]
    assert sorted(os.listdir(tmp_path)) == sorted(f"{detector}{k}-Scenes.csv" for k in range(6)) + ["dump-Scenes.csv"]      # no tmp file stays


def test_default_name_and_refusals(tool, movie, tmp_path):
    mkv, npy, frames, want = movie
    before = sorted(os.listdir(os.path.dirname(mkv)))
    with pytest.raises(ValueError, match="--fps is needed"):
        tool.main(["--color_video", npy])
    with pytest.raises(ValueError, match="decodes .mkv inputs"):
        tool.main(["--color_video", npy, "--fps", "24", "--video_decoder", "device"])
    with pytest.raises(FileNotFoundError):
        tool.main(["--color_video", str(tmp_path / "none.mkv")])
    with pytest.raises(ValueError, match="leaves no image"):
        tool.main(["--color_video", mkv, "--downscale", "100"])
    assert sorted(os.listdir(os.path.dirname(mkv))) == before and os.listdir(tmp_path) == []
    assert tool.main(["--color_video", mkv]) == 0
    assert _read(os.path.join(os.path.dirname(mkv), "movie-Scenes.csv")) == want["adaptive"]
    os.remove(os.path.join(os.path.dirname(mkv), "movie-Scenes.csv"))


def test_the_wrapper_checks_its_tensors(tool, movie):
    import torch
    from metric_depth_video_toolbox_amd import _lib
    mkv, npy, frames, want = movie
    ctx = _lib.Context(torch.cuda.current_device(), 16, 16)
    try:
        d = torch.from_numpy(frames[:4]).cuda()
        got = tool.frame_sums(ctx, d[1:], d[0]).cpu().tolist()
        assert got == sr.frame_sums(frames[1:4], frames[0])
        assert tool.frame_sums(ctx, d[:, :, :40], None, 2).cpu().tolist() == sr.frame_sums(frames[:4, :, :40], factor=2)      # a strided view
        with pytest.raises(TypeError, match="frames"):
            tool.frame_sums(ctx, d.float())
        with pytest.raises(ValueError, match="prev"):
            tool.frame_sums(ctx, d, d[0, :8])
        with pytest.raises(ValueError, match="no pair"):
            tool.frame_sums(ctx, d[:1])
        with pytest.raises(ValueError, match="frames"):
            tool.frame_sums(ctx, torch.from_numpy(frames[:2]))
    finally:
        ctx.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return _tool("movie_2_3D")


def _frames(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        out = np.empty((r.frames, r.height, r.width, 3), np.uint8)
        for k in range(r.frames):
            assert r.read_into(out[k])
        return out


def _stamps(d):
    return {f: os.stat(os.path.join(d, f)).st_mtime_ns for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("codecs", [("host", "host"), ("device", "device")])
def test_step_1_cuts_the_movie_at_the_csv(driver, movie, tmp_path, codecs):
    from metric_depth_video_toolbox_amd import movie_2_3D as host, scene_detect as sd
    mkv, npy, frames, want = movie
    out = str(tmp_path / "out")
    csv_path = sd.write_scene_csv(str(tmp_path / "movie-Scenes.csv"), [(0, 16), (16, 32), (32, 40)], FPS)
    args = host.build_parser().parse_args(["--color_video", mkv, "--scene_file", csv_path, "--output_dir", out, "--video_decoder", codecs[0],
                                           "--video_encoder", codecs[1]])
    os.makedirs(out)
    scenes = host.plan_scene_files(host.load_and_split_scenes(csv_path, ",", 1500), out, -1)
    log = []
    driver.step1_scene_clips(args, scenes, log)
    assert log == [(1, "1", "scene_clip"), (1, "2", "scene_clip"), (1, "3", "scene_clip")]
    assert sorted(os.listdir(out)) == ["scene_1.mkv", "scene_2.mkv", "scene_3.mkv"]
    for k, (a, b) in enumerate(((0, 16), (16, 32), (32, 40)), start=1):
        assert np.array_equal(_frames(os.path.join(out, f"scene_{k}.mkv")), frames[a:b])
    before, log = _stamps(out), []
    driver.step1_scene_clips(args, scenes, log)
    assert log == [] and _stamps(out) == before          # a second run writes nothing
    # a scene list that does not fit the movie is refused before a clip is written
    os.remove(os.path.join(out, "scene_1.mkv"))
    bad = sd.write_scene_csv(str(tmp_path / "bad.csv"), [(0, 41)], FPS)
    with pytest.raises(ValueError, match="do not lie in a movie of 40 frames"):
        driver.step1_scene_clips(args, host.plan_scene_files(host.load_and_split_scenes(bad, ",", 1500), out, -1), [])
    assert sorted(os.listdir(out)) == ["scene_2.mkv", "scene_3.mkv"]


def test_the_whole_pipeline_with_stub_generators(driver, tmp_path):
    """24 frames of 32 x 24, two scenes of 15 and 9 (the detectors' min_scene_len is 15); da3 and mask stubs, --infill_engine normals.  Resume: by the reference's rule
    (m23d:270) a scene whose _infilled file exists is finished whether or not its _stereo file does, so deleting the scene's
    _stereo.mkv alone reruns nothing; deleting it with the two files named after it (_infillmask, _infilled) redoes exactly that
    scene's steps 5 and 6 and the join."""
    import scene_stub_models as stubs
    from metric_depth_video_toolbox_amd import movie_2_3D as host, scene_detect as sd, video_io
    rng = np.random.default_rng(24)
    base = np.array([[235, 200, 30], [40, 60, 210]], np.int64)
    clip = np.clip(base[(np.arange(24) >= 15).astype(int)][:, None, None, :] + rng.integers(-6, 7, (24, 24, 32, 3)), 0, 255).astype(np.uint8)
    mkv, out = str(tmp_path / "film.mkv"), str(tmp_path / "out")
    with video_io.VideoWriter(mkv, 32, 24, FPS) as w:
        for f in clip:
            w.write(f)
    argv = ["--color_video", mkv, "--output_dir", out, "--infill_engine", "normals", "--depth_generator", "scene_stub_models:da3",
            "--mask_generator", "scene_stub_models:mask"]
    result, log = driver.run(host.build_parser().parse_args(argv))
    assert result == os.path.join(out, "film.mkv_SBS.mkv")
    assert open(os.path.join(out, "film-Scenes.csv"), newline="").read() == sr.csv_text([(0, 15), (15, 24)], FPS)
    per_scene = [(1, "scene_clip"), (2, "video_da3"), (3, "generate_video_mask"), (4, "find_convergence_depth"), (5, "stereo_rerender"), (6, "basic_nomal_infill")]
    assert sorted(log) == sorted([(0, "all", "scene_detect"), (7, "all", "join")] + [(s, k, t) for k in ("1", "2") for s, t in per_scene])
    assert [s for s, _, _ in log] == sorted(s for s, _, _ in log)                  # step by step over the scenes
    assert stubs.CALLS["da3"] == 2 and stubs.CALLS["mask"] >= 2
    scenes = host.plan_scene_files(host.load_and_split_scenes(os.path.join(out, "film-Scenes.csv"), ",", 1500), out, -1)
    for s in scenes:                                      # every file the reference's plan names
        for key in ("scene_video_file", "depth_video_file", "mask_video_file", "xfovs_file", "sbs", "sbs_infill", "infilled"):
            assert os.path.isfile(s[key]), s[key]
        assert os.path.isfile(s["depth_video_file"] + "_convergence_depths.json") and s["finished"]
    assert not [f for f in os.listdir(out) if "_tmp" in f]
    joined = _frames(result)
    parts = [_frames(s["infilled"]) for s in scenes]
    assert joined.shape == (24, 24, 64, 3) and np.array_equal(joined, np.concatenate(parts))
    assert np.array_equal(_frames(scenes[1]["scene_video_file"]), clip[15:])
    # a rerun does nothing
    before = _stamps(out)
    result, log = driver.run(host.build_parser().parse_args(argv))
    assert log == [] and _stamps(out) == before
    # the _stereo file alone: the scene stays finished (the reference's rule)
    os.remove(scenes[1]["sbs"])
    result, log = driver.run(host.build_parser().parse_args(argv))
    assert log == []
    # with the files named after it: steps 5-7 of that scene, nothing of the other
    os.remove(scenes[1]["sbs_infill"])
    os.remove(scenes[1]["infilled"])
    calls = dict(stubs.CALLS)
    result, log = driver.run(host.build_parser().parse_args(argv))
    assert log == [(5, "2", "stereo_rerender"), (6, "2", "basic_nomal_infill"), (7, "all", "join")] and stubs.CALLS == calls
    after = _stamps(out)
    changed = sorted(f for f in after if after[f] != before.get(f))
    assert changed == sorted(os.path.basename(p) for p in (scenes[1]["sbs"], scenes[1]["sbs"] + "_holemask.mkv", scenes[1]["sbs_infill"], scenes[1]["infilled"], result))      # (_holemask: the render's own extra)
    assert np.array_equal(_frames(result), joined)
    # --no_render stops after step 4
    out2 = str(tmp_path / "out2")
    result, log = driver.run(host.build_parser().parse_args(argv[:2] + ["--output_dir", out2, "--no_render", "--end_scene", "1"] + argv[6:]))
    assert result is None and [s for s, _, _ in log] == [0, 1, 2, 3, 4]
    assert not [f for f in os.listdir(out2) if "stereo" in f or "SBS" in f]
