"""tools/video_da3.py end to end on a 48 x 32 colour clip of 23 frames with a stub in the model's place: the three files it writes
against the NumPy restatement of the whole step (tests/depth_sink_ref.run_step) -- the depth video byte for byte, the fields of view
equal, the poses to 1e-9 -- with arbitrary drifts between the model's calls and with drifts whose factor is exact; the device decoder
with the device encoder; --max_frames; a .txt list; and a generator that breaks its contract.

The stub.  Its 12 x 8 depth is a function of the frame's bytes (the red byte of every fourth pixel) times a drift that changes with
every call, as a model's scale does from batch to batch.  Its poses are one trajectory (the frame's number is its first green byte),
re-gauged per call by a rigid transform of the world and the same drift: what the step's factor and alignment are there to undo."""
import importlib.util
import json
import os

import numpy as np
import pytest

import depth_sink_ref as dr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N, W, H = 23, 48, 32
FLAGS = ["--images_per_batch", "8", "--batch_overlap", "2", "--nr_of_ref_frames", "3", "--max_depth", "20"]
STEP = dict(max_depth=20, images_per_batch=8, batch_overlap=2, nr_of_ref_frames=3)


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("video_da3_tool", os.path.join(REPO, "tools", "video_da3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def trajectory(i):
    """World-to-camera [3, 4] of frame i: a camera on a rising spiral (no three centres on a line), turning as it goes."""
    c = np.array([np.cos(0.31 * i) * (1.0 + 0.05 * i), 0.2 * i + 0.3 * np.sin(0.9 * i), np.sin(0.31 * i) * 1.3])
    R = _rot([0.2, 1.0, 0.1], 0.07 * i)
    return np.hstack([R, (-R @ c)[:, None]])


class Stub:
    """infer(frames, resolution) on host arrays; call k drifts by drifts[k] in a world moved by gauges[k]."""

    def __init__(self, drifts, integer=False):
        self.drifts, self.integer, self.calls, self.seen = list(drifts), integer, 0, []
        self.gauges = [(np.eye(3), np.zeros(3))] + [(_rot([1.0, 0.3 * k, -0.5], 0.4 * k), np.array([0.5 * k, -1.0, 0.25 * k])) for k in range(1, len(self.drifts))]

    def __call__(self, frames, resolution):
        frames = np.asarray(frames)
        d, (Rg, tg) = self.drifts[self.calls], self.gauges[self.calls]
        self.calls += 1
        self.seen.append((frames.shape, resolution))
        red = frames[:, ::4, ::4, 0].astype(F)                      # [T, 8, 12]
        base = (np.mod(red, F(15)) + F(1)) if self.integer else (red / F(16) + F(0.5))
        depth = (base * F(d)).astype(F)
        ext = []
        for i in frames[:, 0, 0, 1]:
            E = trajectory(int(i))
            R = E[:, :3] @ Rg.T
            ext.append(np.hstack([R, (d * (E[:, 3] - R @ tg))[:, None]]))
        fx = 40.0 + frames[:, 0, 0, 1].astype(np.float64)
        intr = np.stack([np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]) for f in fx]).astype(F)
        return depth, np.stack(ext), intr


class DeviceStub(Stub):
    """The same model under the generator's contract: uint8 CUDA frames in; the depth back on the device, the intrinsics as a CUDA
    tensor too, the extrinsics on the host."""

    def __call__(self, frames, resolution):
        import torch
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3
        depth, ext, intr = super().__call__(frames.cpu().numpy(), resolution)
        return torch.from_numpy(depth).to(frames.device), ext, torch.from_numpy(intr).to(frames.device)


def _clip(d, name="x.mkv", seed=3):
    from metric_depth_video_toolbox_amd import video_io
    color = np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    color[:, 0, 0, 1] = np.arange(N)
    path = str(d / name)
    with video_io.VideoWriter(path, W, H, 24.0) as wr:
        for f in color:
            wr.write(f)
    return path, color


def _read(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        frames = np.empty((r.frames, r.height, r.width, 3), np.uint8)
        for k in range(r.frames):
            assert r.read_into(frames[k])
        return frames


def _args(path, *more):
    from metric_depth_video_toolbox_amd import video_da3
    return video_da3.build_parser().parse_args(["--color_video", path] + FLAGS + list(more))


DRIFTS = (1.0, 1.2345678, 0.8123)


@pytest.fixture(scope="module")
def arbitrary(tool, tmp_path_factory):
    """The clip through the tool on the host route with arbitrary drifts, and the restatement of it: computed once, shared."""
    d = tmp_path_factory.mktemp("da3")
    path, color = _clip(d)
    stub = DeviceStub(DRIFTS)
    written = tool.run(_args(path), stub)
    want = dr.run_step(color, Stub(DRIFTS), resolution=504, **STEP)
    return d, path, color, written, stub, want


def test_the_three_files_equal_the_restatement(arbitrary):
    d, path, color, written, stub, (codes, xfovs, transformations, factors) = arbitrary
    assert written == [path + "_depth.mkv"]
    assert sorted(os.listdir(d)) == ["x.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_transformations.json", "x.mkv_depth.mkv_xfovs.json"]
    # references 0, 7, 14, 21 (23 // 3 = 7); then the overlap of 2 and 8 new frames
    assert [s for s, _ in stub.seen] == [(4 + 8, H, W, 3), (4 + 2 + 8, H, W, 3), (4 + 2 + 7, H, W, 3)] and all(r == 504 for _, r in stub.seen)
    got = _read(path + "_depth.mkv")
    assert got.shape == (N, H, W, 3) and np.array_equal(got, codes)
    assert json.load(open(path + "_depth.mkv_xfovs.json")) == xfovs and len(xfovs) == N
    T = np.array(json.load(open(path + "_depth.mkv_transformations.json")))
    assert T.shape == (N, 4, 4) and np.abs(T - transformations).max() < 1e-9
    assert len(factors) == 2 and all(abs(f * dk - 1) < 0.05 for f, dk in zip(factors, DRIFTS[1:]))


@pytest.mark.parametrize("decoder", ["device", "device_all"])
def test_the_device_decoder_with_the_device_encoder_gives_the_host_routes_bytes(tool, arbitrary, tmp_path, decoder):
    d, path, color, _, _, want = arbitrary
    import shutil
    clip = str(tmp_path / "x.mkv")
    shutil.copy(path, clip)
    tool.run(_args(clip, "--video_decoder", decoder, "--video_encoder", "device"), DeviceStub(DRIFTS))
    for tail in ("_depth.mkv", "_depth.mkv_xfovs.json", "_depth.mkv_transformations.json"):
        assert open(clip + tail, "rb").read() == open(path + tail, "rb").read(), tail


def test_exact_drifts_give_the_inverse_factor_and_the_ungauged_trajectory(tool, tmp_path):
    """Integer depths 1 .. 15 and drifts 2 and 0.5: every float32 sum stays below 2^24, so it is exact."""
    path, color = _clip(tmp_path, seed=4)
    drifts = (1.0, 2.0, 0.5)
    tool.run(_args(path), DeviceStub(drifts, integer=True))
    codes, xfovs, transformations, factors = dr.run_step(color, Stub(drifts, integer=True), **STEP)
    assert [float(f) for f in factors] == [0.5, 2.0]
    assert np.array_equal(_read(path + "_depth.mkv"), codes)
    # the depth video is the un-drifted model's: every batch at the first call's scale
    plain = Stub((1.0,), integer=True)(color, 504)[0]
    assert np.array_equal(codes, dr.sink(plain, 20, (W, H))[0])
    T = np.array(json.load(open(path + "_depth.mkv_transformations.json")))
    want = np.stack([np.linalg.inv(dr.h4(trajectory(i))) for i in range(N)])
    assert np.abs(T - want).max() < 1e-9
    assert json.load(open(path + "_depth.mkv_xfovs.json")) == xfovs


def test_max_frames_takes_the_first_frames(tool, arbitrary, tmp_path):
    _, path, color, _, _, _ = arbitrary
    import shutil
    clip = str(tmp_path / "y.mkv")
    shutil.copy(path, clip)
    tool.run(_args(clip, "--max_frames", "11"), DeviceStub(DRIFTS))
    want = dr.run_step(color[:11], Stub(DRIFTS), **STEP)
    got = _read(clip + "_depth.mkv")
    assert got.shape[0] == 11 and np.array_equal(got, want[0])
    assert len(json.load(open(clip + "_depth.mkv_xfovs.json"))) == 11 and len(json.load(open(clip + "_depth.mkv_transformations.json"))) == 11


def test_a_txt_list_runs_each_entry_and_a_npy_dump_gives_npy_frames(tool, arbitrary, tmp_path):
    _, path, color, _, _, want = arbitrary
    import shutil
    a, b = str(tmp_path / "a.mkv"), str(tmp_path / "b.npy")
    shutil.copy(path, a)
    np.save(b, color[:9])
    lst = tmp_path / "clips.txt"
    lst.write_text(f"# two clips\n{a}\n\n{b}\n")
    calls = []

    def infer(frames, resolution):                                  # a fresh stub per clip: a clip's first call ends inside its first batch
        if int(frames[-1, 0, 0, 1]) < 8:
            calls.append(DeviceStub(DRIFTS))
        return calls[-1](frames, resolution)
    written = tool.run(_args(str(lst)), infer)
    assert written == [a + "_depth.mkv", b + "_depth.npy"] and len(calls) == 2
    assert np.array_equal(_read(a + "_depth.mkv"), want[0])
    assert np.array_equal(np.load(b + "_depth.npy"), dr.run_step(color[:9], Stub(DRIFTS), **STEP)[0])
    assert os.path.exists(b + "_depth.npy_xfovs.json") and not os.path.exists(b + "_tmp_depth.npy")


def test_a_generator_that_breaks_its_contract_raises_before_a_launch(tool, arbitrary, tmp_path):
    import shutil
    import torch
    _, path, _, _, _, _ = arbitrary
    clip = str(tmp_path / "z.mkv")
    shutil.copy(path, clip)
    good = DeviceStub(DRIFTS)

    def broken(how):
        def infer(frames, resolution):
            depth, ext, intr = DeviceStub(DRIFTS)(frames, resolution)
            if how == "dtype":
                depth = depth.double()
            elif how == "shape":
                depth = depth[1:]
            elif how == "host":
                depth = depth.cpu()
            elif how == "poses":
                ext = ext[:, :2]
            elif how == "int poses":
                ext = ext.astype(np.int64)
            elif how == "pair":
                return depth, ext
            return depth, ext, intr
        return infer
    launched = []
    real = tool.depth_video_codes
    tool.depth_video_codes = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        for how, error in (("dtype", TypeError), ("shape", ValueError), ("host", ValueError), ("poses", ValueError), ("int poses", TypeError),
                           ("pair", TypeError)):
            with pytest.raises(error):
                tool.run(_args(clip), broken(how))
            assert not launched and os.listdir(tmp_path) == ["z.mkv"], how       # nothing launched, no file left
        tool.run(_args(clip), good)
        assert len(launched) == 3 and torch.cuda.is_available()
    finally:
        tool.depth_video_codes = real


def test_a_generator_whose_depth_is_strided_in_rows_and_frames_gives_the_same_files(tool, arbitrary, tmp_path):
    """INTEGRATION.md lets the depth's rows and frames be strided: the fit and the sink take the view as it is."""
    import shutil
    import torch
    _, path, _, _, _, _ = arbitrary
    clip = str(tmp_path / "s.mkv")
    shutil.copy(path, clip)
    inner = DeviceStub(DRIFTS)
    strides = []

    def infer(frames, resolution):
        depth, ext, intr = inner(frames, resolution)
        T, h, w = depth.shape
        buf = torch.full((T, h + 3, w + 5), float("nan"), dtype=torch.float32, device=depth.device)      # padded rows, gapped frames
        view = buf[:, 1:1 + h, 2:2 + w]
        view.copy_(depth)
        strides.append(tuple(view.stride()))
        return view, ext, intr
    tool.run(_args(clip), infer)
    assert strides and all(s == ((8 + 3) * (12 + 5), 12 + 5, 1) for s in strides)
    for tail in ("_depth.mkv", "_depth.mkv_xfovs.json", "_depth.mkv_transformations.json"):
        assert open(clip + tail, "rb").read() == open(path + tail, "rb").read(), tail
