"""tools/sam_track_video.py end to end on 12-frame clips with a stub in the tracker's place (tests/megasam_stub_models.py): the
transformation file value for value and the two videos byte for byte equal to the NumPy restatement of the whole step
(tests/megasam_ref.run_step), with the host and the device codecs, with and without --mask_video, with --max_frames 3 and with a
colour video one frame longer (the track_final call); what the stub was handed equals the restatement's model inputs bit for bit; no
tmp file is left; the posed render accepts the transformation file.

The clips are 640 x 360, not smaller: stv:134-136 gives the tracker 591 x 332 whatever the video's size, and a video below that would
ask cv2.resize(INTER_AREA) to enlarge, which include/mdvt_megasam.h refuses."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import megasam_ref as gr
import megasam_stub_models as stub

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N, W, H = 12, 640, 360
MAX_DEPTH, BATCH, XFOV = 20, 5, 60.0


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("sam_track_video_tool", os.path.join(REPO, "tools", "sam_track_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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
def clips(tmp_path_factory):
    """A colour video of N + 1 frames (its first N: the equal-length clip), a depth video and a mask video of N, in files, and as arrays."""
    d = tmp_path_factory.mktemp("megasam")
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    color = np.stack([np.stack([(xx + 7 * k) % 256, (yy * 2 + 3 * k) % 256, (xx + yy + 11 * k) % 256], -1) for k in range(N + 1)]).astype(np.uint8)
    color[:, ::9, ::7] = rng.integers(0, 256, color[:, ::9, ::7].shape, dtype=np.uint8)
    code = ((xx * 90 + yy * 140 + 1500 * np.arange(N)[:, None, None]) % 65536).astype(np.uint32)       # 16-bit depth codes
    depth = np.stack([code >> 8, (code >> 8) ^ (np.arange(N)[:, None, None] % 2 * 0x33), code & 0xFF], -1).astype(np.uint8)   # odd frames: G differs from R
    mask = np.zeros((N, H, W, 3), np.uint8)
    for k in range(N):
        mask[k, 40 + 5 * k:200 + 5 * k, 100 + 20 * k:300 + 20 * k] = 255
        mask[k, 250:300, 50:400] = (xx[250:300, 50:400, None] % 256).astype(np.uint8)               # greys
    files = dict(color=_write(str(d / "x.mkv"), color[:N]), longer=_write(str(d / "x_longer.mkv"), color),
                 depth=_write(str(d / "x.mkv_depth.mkv"), depth), mask=_write(str(d / "x_mask.mkv"), mask))
    return d, files, dict(color=color, depth=depth, mask=mask)


def _args(color, depth, *more):
    from metric_depth_video_toolbox_amd import sam_track
    return sam_track.build_parser().parse_args(["--color_video", color, "--depth_video", depth, "--xfov", str(XFOV), "--max_depth", str(MAX_DEPTH),
                                                "--batch", str(BATCH)] + list(more))


def _run(tool, files, where, color="color", mask=False, more=()):
    """The tool on copies of the clips in `where` -> (the depth video's path there, what it wrote, the tracker it made)."""
    os.makedirs(where, exist_ok=True)
    c = shutil.copy(files[color], os.path.join(where, "x.mkv"))
    d = shutil.copy(files["depth"], os.path.join(where, "x.mkv_depth.mkv"))
    extra = list(more)
    if mask:
        extra += ["--mask_video", shutil.copy(files["mask"], os.path.join(where, "x_mask.mkv"))]
    before = len(stub.TRACKERS)
    written = tool.run(_args(c, d, *extra), stub.make_tracker)
    assert len(stub.TRACKERS) == before + 1
    return d, written, stub.TRACKERS[-1]


def _restated(arrays, n_color=N, mask=False, max_frames=-1):
    return gr.run_step(arrays["color"][:n_color], arrays["depth"], arrays["mask"] if mask else None, stub.core, max_frames=max_frames,
                       max_depth=MAX_DEPTH, xfov=XFOV)


def _check(d, written, tracker, want, files_in_dir):
    assert written == {"json": d + "_transformations.json", "depth": d + "_megasam.mkv", "motion": d + "_megasam_motion.mkv"}
    assert sorted(os.listdir(os.path.dirname(d))) == sorted(files_in_dir + [os.path.basename(p) for p in written.values()])     # no tmp file is left
    t = len(want["items"])
    assert tracker.image_size == [328, 584] and len(tracker.handed) == t and tracker.final == want["final"]
    for got, item in zip(tracker.handed, want["items"]):            # what the tracker was handed: the restatement's model inputs, bit for bit
        assert got[0] == item[0]
        for a, b in zip(got[1:], item[1:]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), item[0]
    T = np.array(json.load(open(written["json"])))
    assert T.shape == (t + 1, 4, 4) and np.array_equal(T, want["transformations"]) and np.array_equal(T[0], np.eye(4))
    for what, key in (("depth", "depth_frames"), ("motion", "motion_frames")):
        got = _read(written[what])
        assert got.shape == (t, H, W, 3) and np.array_equal(got, want[key]), what


@pytest.fixture(scope="module")
def host_route(tool, clips):
    """Equal lengths, no mask, the host codecs, and the restatement: computed once, shared."""
    d, files, arrays = clips
    return _run(tool, files, str(d / "host")) + (_restated(arrays),)


def test_the_three_files_equal_the_restatement(host_route):
    d, written, tracker, want = host_route
    _check(d, written, tracker, want, ["x.mkv", "x.mkv_depth.mkv"])
    assert len(want["items"]) == N - 1 and want["final"] is None    # equal lengths: the last frame is never handed over, and no track_final
    assert all(np.all(item[4] == 1) for item in tracker.handed)     # without a mask video: ones
    assert tracker.optimize_intrinsic is False


def test_the_device_codecs_and_a_mask_video(tool, clips, host_route, tmp_path):
    d0, files, arrays = clips
    d, written, tracker = _run(tool, files, str(tmp_path / "dev"), mask=True,
                               more=["--video_decoder", "device", "--video_encoder", "device", "--optimize_intrinsic"])
    want = _restated(arrays, mask=True)
    _check(d, written, tracker, want, ["x.mkv", "x.mkv_depth.mkv", "x_mask.mkv"])
    assert tracker.optimize_intrinsic is True
    assert not np.array_equal(want["motion_frames"], host_route[3]["motion_frames"])       # the mask reached the tracker
    motion = want["motion_frames"]
    assert np.array_equal(motion[..., 0], motion[..., 2]) and motion.min() == 0 and motion.max() == 255      # a grey video that reaches both clips
    # the device codecs alone, without the mask, give the host route's files byte for byte
    d2, written2, _ = _run(tool, files, str(tmp_path / "dev2"), more=["--video_decoder", "device_all", "--video_encoder", "device"])
    for what in ("json", "depth", "motion"):
        assert open(written2[what], "rb").read() == open(host_route[1][what], "rb").read(), what


def test_max_frames_3_hands_over_five_frames(tool, clips, tmp_path):
    _, files, arrays = clips
    d, written, tracker = _run(tool, files, str(tmp_path / "m3"), mask=True, more=["--max_frames", "3"])
    want = _restated(arrays, mask=True, max_frames=3)
    assert len(want["items"]) == 5 and want["final"] == 4           # M + 2 frames, the last through track_final
    _check(d, written, tracker, want, ["x.mkv", "x.mkv_depth.mkv", "x_mask.mkv"])


def test_a_longer_colour_video_shows_the_track_final_call(tool, clips, tmp_path):
    _, files, arrays = clips
    d, written, tracker = _run(tool, files, str(tmp_path / "longer"), color="longer")
    want = _restated(arrays, n_color=N + 1)
    assert len(want["items"]) == N and want["final"] == N - 1
    _check(d, written, tracker, want, ["x.mkv", "x.mkv_depth.mkv"])


def test_the_posed_render_accepts_the_transformation_file(host_route, tmp_path):
    from metric_depth_video_toolbox_amd import clip
    d, written, _, want = host_route
    cl = clip.load_clip_parameters(N, W, H, xfov=XFOV, transformation_file=written["json"])
    assert cl.transformations is not None and len(cl.transformations) == N
    depth, color = shutil.copy(d, str(tmp_path / "x.mkv_depth.mkv")), shutil.copy(os.path.join(os.path.dirname(d), "x.mkv"), str(tmp_path / "x.mkv"))
    stats, final = clip.run(depth, color, batch=2, max_frames=2, xfov=XFOV, max_depth=MAX_DEPTH, transformation_file=written["json"],
                            transformation_lock_frame=1, pupillary_distance=65, render_as_pointcloud=True)
    assert os.path.exists(final) and int(stats[:, 0].sum()) == 2 and _read(final).shape == (2, H, 2 * W, 3)
