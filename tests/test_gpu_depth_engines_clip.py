"""tools/depth_engine_video.py and tools/upscale_depth_promptda.py end to end on a 64 x 36 colour clip of 12 frames with stubs in the
models' places: the depth video byte for byte and the x-fov list equal to the NumPy restatement of the whole step
(tests/depth_engines_ref.run_engine / run_promptda), the host and the device codecs giving the same files, --max_frames, the camera a
model is handed with --xfov, no tmp file left.

The stubs are deterministic functions of the frames they are handed (so a frame that reached the model changed shows up in the
files).  unik3d: a 16 x 12 depth from the red plane, and a full-size point map of a pinhole camera whose focal length is 40 + the
first red byte, its depth the green plane.  moge: a depth from the red plane with NaN where blue is high, float32 intrinsics from
the first green value.  depthpro: a depth that exceeds max_depth (the sink's clip), a focal length from the first blue byte.
PromptDA: a function of both of its inputs."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import depth_engines_ref as er

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N, W, H = 12, 64, 36
MAX_DEPTH, BATCH = 20, 5
ENGINES = ("unik3d", "moge", "depthpro")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool("depth_engine_video")


@pytest.fixture(scope="module")
def promptda_tool():
    return _tool("upscale_depth_promptda")


# ---- the stubs, on host arrays ----------------------------------------------------------------------------------------------------
def stub_unik3d(frames):
    """uint8 [n, 3, H, W] -> depth [n, 12, 16], points [n, 3, H, W]."""
    assert frames.dtype == np.uint8 and frames.shape[1:] == (3, H, W)
    depth = (frames[:, 0, ::3, ::4].astype(F) / F(16) + F(0.5)).astype(F)
    f = (F(40) + frames[:, 0, 0, 0].astype(F))[:, None, None]
    v, u = np.mgrid[0:H, 0:W].astype(F)
    Z = (frames[:, 1].astype(F) / F(32) + F(1)).astype(F)
    X = ((u - F(W / 2)) * Z / f).astype(F)
    Y = ((v - F(H / 2)) * Z / f).astype(F)
    return dict(depth=depth, points=np.stack([X, Y, Z], axis=1))


def stub_moge(frames):
    """float32 [n, 3, H, W] in [0, 1] -> depth [n, 12, 16] with NaN, intrinsics [n, 3, 3]."""
    assert frames.dtype == np.float32 and frames.shape[1:] == (3, H, W) and frames.max() <= 1.0
    depth = (frames[:, 0, ::3, ::4] * F(24) + F(0.5)).astype(F)
    depth[frames[:, 2, ::3, ::4] > F(0.9)] = np.nan
    K = np.tile(np.eye(3, dtype=F), (len(frames), 1, 1))
    K[:, 0, 0] = F(0.5) + frames[:, 1, 0, 0]
    K[:, 1, 1] = F(0.75) + frames[:, 1, 0, 0]
    K[:, 0, 2] = K[:, 1, 2] = F(0.5)
    return dict(depth=depth, intrinsics=K)


def stub_depthpro(frames):
    assert frames.dtype == np.uint8 and frames.shape[1:] == (3, H, W)
    depth = (frames[:, 0, ::3, ::4].astype(F) / F(8)).astype(F)      # up to 31.9: beyond max_depth
    return dict(depth=depth, focallength_px=(F(50) + frames[:, 2, 0, 0].astype(F)).astype(F))


STUBS = {"unik3d": stub_unik3d, "moge": stub_moge, "depthpro": stub_depthpro}


def stub_promptda(rgb, prompt):
    """float32 [k, 3, 42, 70], [k, 1, 192, 256] -> [k, 42, 70]."""
    assert rgb.dtype == np.float32 and rgb.shape[1:] == (3, 42, 70) and prompt.dtype == np.float32 and prompt.shape[1:] == (1, 192, 256)
    return (rgb[:, 1] * F(5) + prompt[:, 0, 40:82:1, 100:170] * F(0.5)).astype(F)


class OnDevice:
    """A stub under the generators' contract: CUDA tensors in, CUDA tensors out; it remembers what it was handed."""

    def __init__(self, fn):
        self.fn, self.seen, self.second = fn, [], []

    def __call__(self, frames, second):
        import torch
        assert frames.is_cuda and frames.is_contiguous()
        self.seen.append(tuple(frames.shape))
        if isinstance(second, torch.Tensor):
            assert second.is_cuda
            got = self.fn(frames.cpu().numpy(), second.cpu().numpy())
            return torch.from_numpy(got).to(frames.device)
        self.second.append(second)
        return {k: torch.from_numpy(v).to(frames.device) for k, v in self.fn(frames.cpu().numpy()).items()}


# ---- the clips ----------------------------------------------------------------------------------------------------------------------
def _write(path, frames, fps=24.0):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoWriter(path, frames.shape[2], frames.shape[1], fps) as wr:
        for f in frames:
            wr.write(f)
    return path


def _read(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        frames = np.empty((r.frames, r.height, r.width, 3), np.uint8)
        for k in range(r.frames):
            assert r.read_into(frames[k])
        return frames


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("engines")
    rng = np.random.default_rng(7)
    color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    color[:, 0, 0] = np.stack([np.arange(N) * 7, np.arange(N) * 11 + 3, np.arange(N) * 5 + 1], axis=-1)
    code = rng.integers(0, 1 << 16, (N, 24, 40))
    depth = np.stack([code >> 8, code >> 8, code & 0xFF], axis=-1).astype(np.uint8)      # a 40 x 24 depth video
    return d, _write(str(d / "x.mkv"), color), color, _write(str(d / "d.mkv"), depth), depth


def _args(engine, path, *more):
    from metric_depth_video_toolbox_amd import depth_engines
    return depth_engines.build_engine_parser().parse_args(["--engine", engine, "--color_video", path, "--max_depth", str(MAX_DEPTH),
                                                           "--batch", str(BATCH)] + list(more))


@pytest.fixture(scope="module")
def host_route(tool, clip):
    """Each engine through the tool on the host codecs, in a directory of its own, and the restatement: computed once, shared."""
    d, path, color, _, _ = clip
    out = {}
    for engine in ENGINES:
        os.mkdir(d / engine)
        mine = shutil.copy(path, str(d / engine / "x.mkv"))
        stub = OnDevice(STUBS[engine])
        written = tool.run(_args(engine, mine), stub)
        out[engine] = (mine, written, stub, er.run_engine(color, engine, STUBS[engine], MAX_DEPTH, BATCH))
    return out


@pytest.mark.parametrize("engine", ENGINES)
def test_the_depth_video_and_the_x_fovs_equal_the_restatement(host_route, engine):
    mine, written, stub, (codes, xfovs) = host_route[engine]
    assert written == [mine + "_depth.mkv"]
    assert sorted(os.listdir(os.path.dirname(mine))) == ["x.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_xfovs.json"]      # no tmp file is left
    assert stub.seen == [(5, 3, H, W), (5, 3, H, W), (2, 3, H, W)] and stub.second == [None] * 3
    got = _read(mine + "_depth.mkv")
    assert got.shape == (N, H, W, 3) and np.array_equal(got, codes)
    assert json.load(open(mine + "_depth.mkv_xfovs.json")) == xfovs and len(xfovs) == N and len(set(xfovs)) == N


def test_the_unik3d_x_fovs_are_those_of_the_stubs_focal_lengths(host_route):
    """The point map comes from a known focal length: the estimate's mean returns it to float32 accuracy, and the x-fov follows."""
    xfovs = host_route["unik3d"][3][1]
    for k, fov in enumerate(xfovs):
        f = 40.0 + (k * 7) % 256
        assert abs(fov - np.rad2deg(2 * np.arctan2(W, 2 * f))) < 1e-3, k


def test_moge_codes_nan_as_max_depth_and_depthpro_clips(host_route):
    import metric_align_ref as mr
    top = mr.code(np.full((1, 1), MAX_DEPTH, F), MAX_DEPTH)[1][0, 0]                   # the code of max_depth itself
    codes = host_route["moge"][3][0]
    assert (codes == top).all(-1).any() and (codes[..., 0] < top[0]).any()
    deep = host_route["depthpro"][3][0]
    assert (deep == top).all(-1).mean() > 0.1                       # a third of the depths lie beyond max_depth


@pytest.mark.parametrize("engine,decoder", [("unik3d", "device"), ("moge", "device_all"), ("depthpro", "device")])
def test_the_device_codecs_give_the_host_routes_files(tool, host_route, tmp_path, engine, decoder):
    mine = host_route[engine][0]
    other = shutil.copy(mine, str(tmp_path / "x.mkv"))
    tool.run(_args(engine, other, "--video_decoder", decoder, "--video_encoder", "device"), OnDevice(STUBS[engine]))
    assert sorted(os.listdir(tmp_path)) == ["x.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_xfovs.json"]
    for tail in ("_depth.mkv", "_depth.mkv_xfovs.json"):
        assert open(other + tail, "rb").read() == open(mine + tail, "rb").read(), tail


def test_max_frames_writes_exactly_that_many_and_xfov_reaches_the_model(tool, clip, tmp_path):
    from metric_depth_video_toolbox_amd import depth_engines
    _, path, color, _, _ = clip
    other = shutil.copy(path, str(tmp_path / "y.mkv"))
    stub = OnDevice(stub_unik3d)
    tool.run(_args("unik3d", other, "--max_frames", "7", "--xfov", "60"), stub)
    codes, xfovs = er.run_engine(color[:7], "unik3d", stub_unik3d, MAX_DEPTH, BATCH)
    got = _read(other + "_depth.mkv")
    assert got.shape[0] == 7 and np.array_equal(got, codes) and json.load(open(other + "_depth.mkv_xfovs.json")) == xfovs
    assert stub.seen == [(5, 3, H, W), (2, 3, H, W)]
    cam = depth_engines.requested_camera(60.0, None, W, H)
    assert all(c.dtype == np.float32 and np.array_equal(c, cam) for c in stub.second)      # u3d:143: the float32 camera matrix
    stub = OnDevice(stub_moge)
    tool.run(_args("moge", other, "--max_frames", "3", "--xfov", "60"), stub)
    assert _read(other + "_depth.mkv").shape[0] == 3
    assert all(isinstance(v, np.float32) and abs(float(v) - 60.0) < 1e-4 for v in stub.second)      # mge:136, 162: fov_x


def test_a_generator_that_breaks_its_contract_raises_and_leaves_no_file(tool, clip, tmp_path):
    _, path, _, _, _ = clip
    other = shutil.copy(path, str(tmp_path / "z.mkv"))

    def no_points(frames, cam):
        got = OnDevice(stub_unik3d)(frames, cam)
        del got["points"]
        return got

    def small_points(frames, cam):
        got = OnDevice(stub_unik3d)(frames, cam)
        got["points"] = got["points"][:, :, ::2]
        return got

    def double_depth(frames, cam):
        got = OnDevice(stub_unik3d)(frames, cam)
        got["depth"] = got["depth"].double()
        return got
    for infer, error in ((no_points, TypeError), (small_points, ValueError), (double_depth, TypeError)):
        with pytest.raises(error):
            tool.run(_args("unik3d", other), infer)
        assert os.listdir(tmp_path) == ["z.mkv"]


def test_the_x_fov_list_is_written_before_the_depth_video_gets_its_name(tool, clip, tmp_path, monkeypatch):
    """u3d:185-191: the list, then the video.  A list that cannot be written leaves neither file; the list that is written finds the
    depth video still under its tmp name."""
    from metric_depth_video_toolbox_amd import depth_engines
    _, path, _, _, _ = clip
    other = shutil.copy(path, str(tmp_path / "w.mkv"))
    real, seen = depth_engines.write_xfovs, []

    def failing(xfov_file, xfovs):
        raise OSError("the disk is full")
    monkeypatch.setattr(depth_engines, "write_xfovs", failing)
    with pytest.raises(OSError, match="disk is full"):
        tool.run(_args("unik3d", other), OnDevice(stub_unik3d))
    assert os.listdir(tmp_path) == ["w.mkv"]

    def watching(xfov_file, xfovs):
        seen.append(sorted(os.listdir(tmp_path)))
        real(xfov_file, xfovs)
    monkeypatch.setattr(depth_engines, "write_xfovs", watching)
    tool.run(_args("unik3d", other), OnDevice(stub_unik3d))
    assert seen == [["w.mkv", "w.mkv_tmp_depth.mkv"]]
    assert sorted(os.listdir(tmp_path)) == ["w.mkv", "w.mkv_depth.mkv", "w.mkv_depth.mkv_xfovs.json"]


# ---- PromptDA -----------------------------------------------------------------------------------------------------------------------
def _promptda_args(color, depth, *more):
    from metric_depth_video_toolbox_amd import depth_engines
    return depth_engines.build_promptda_parser().parse_args(["--color_video", color, "--depth_video", depth, "--max_depth", str(MAX_DEPTH),
                                                             "--batch", str(BATCH)] + list(more))


def test_promptda_equals_the_restatement_on_host_and_device_codecs(promptda_tool, clip, tmp_path):
    _, path, color, dpath, depth = clip
    want = er.run_promptda(color, depth, stub_promptda, MAX_DEPTH, BATCH)
    files = {}
    for route, more in (("host", ()), ("device", ("--video_decoder", "device", "--video_encoder", "device"))):
        os.mkdir(tmp_path / route)
        c, d = shutil.copy(path, str(tmp_path / route / "x.mkv")), shutil.copy(dpath, str(tmp_path / route / "d.mkv"))
        stub = OnDevice(stub_promptda)
        assert promptda_tool.run(_promptda_args(c, d, *more), stub) == d + "_upscaled.mkv"
        assert sorted(os.listdir(tmp_path / route)) == ["d.mkv", "d.mkv_upscaled.mkv", "x.mkv"]      # no tmp file is left
        assert stub.seen == [(5, 3, 42, 70), (5, 3, 42, 70), (2, 3, 42, 70)]
        got = _read(d + "_upscaled.mkv")
        assert got.shape == (N, H, W, 3) and np.array_equal(got, want), route
        files[route] = open(d + "_upscaled.mkv", "rb").read()
    assert files["host"] == files["device"]
    # --max_frames
    c, d = shutil.copy(path, str(tmp_path / "x.mkv")), shutil.copy(dpath, str(tmp_path / "d.mkv"))
    promptda_tool.run(_promptda_args(c, d, "--max_frames", "6"), OnDevice(stub_promptda))
    assert np.array_equal(_read(d + "_upscaled.mkv"), er.run_promptda(color[:6], depth[:6], stub_promptda, MAX_DEPTH, BATCH))
