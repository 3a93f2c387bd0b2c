"""The viewer's CLI on a 64 x 48, 5-frame .mkv pair with a transformation file: the output file decodes to render_view's frames, the
device decoder and encoder give the host's bytes, and a fully given target launches no centre kernel."""
import json
import os

import numpy as np
import pytest

import test_gpu_view_render as tvr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H, N = 64, 48, 5


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd import clip_io
    d = tmp_path_factory.mktemp("view_clip")
    rng = np.random.default_rng(3)
    depth, color = tvr.scene(rng, N, H, W)
    paths = {}
    for name, frames in (("depth", depth), ("color", color)):
        paths[name] = str(d / f"{name}.mkv")
        sink = clip_io.VideoSink(paths[name], W, H, 24.0)
        sink.write_from(frames, 0, N)
        sink.close()
    Ts = tvr.poses(N)
    paths["T"] = str(d / "t.json")
    with open(paths["T"], "w") as fh:
        json.dump([T.tolist() for T in Ts], fh)
    return paths, depth, color, Ts


def decoded(path):
    from metric_depth_video_toolbox_amd import clip_io
    frames = clip_io.open_frames(path, FileNotFoundError(path))
    try:
        return np.asarray(frames).copy()
    finally:
        for p, _ in clip_io.video_parts(frames):
            p.close()


@pytest.mark.parametrize("pointcloud", [False, True], ids=["mesh", "points"])
def test_the_cli_writes_render_views_frames(clip, pointcloud):
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    from metric_depth_video_toolbox_amd.stereo_rerender import make_frame_params
    paths, depth, color, Ts = clip
    argv = ["--depth_video", paths["depth"], "--color_video", paths["color"], "--xfov", "45", "--render", "--remove_edges",
            "--transformation_file", paths["T"], "--batch", "2", "--x", "0.6", "--y", "0.5", "--z", "-1.2", "--ty", "0.1"]
    out = paths["depth"] + "_render.mkv"
    assert vd.main(argv + (["--render_as_pointcloud"] if pointcloud else [])) == 0
    got = decoded(out)
    host_bytes = open(out, "rb").read()
    r = vd.view_renderer(W, H, device=0, render_as_pointcloud=pointcloud, remove_edges=True)
    try:
        params = [make_frame_params(W, H, xfov=45, master_xfov=45, pupillary_distance=0, transformation=T) for T in Ts]
        d, c = torch.from_numpy(depth).cuda(), torch.from_numpy(color).cuda()
        cen = vd.centers(d, params, r).cpu().numpy()
        cam = vd.camera_position(0.6, 0.5, -1.2)
        views = np.stack([vd.look_at_view(cam, vd.look_at_target(cen[k], ty=0.1)) for k in range(N)])
        want = vd.render_view(d, c, views, params, r)["rgb"].cpu().numpy()
    finally:
        r.close()
    assert got.shape == (N, H, W, 3) and np.array_equal(got, want)
    assert (want == 255).all(axis=-1).any() and not (want == 255).all()      # white holes, and a scene
    # the device decoder and encoder: the same file
    assert vd.main(argv + ["--video_decoder", "device", "--video_encoder", "device"] + (["--render_as_pointcloud"] if pointcloud else [])) == 0
    assert open(out, "rb").read() == host_bytes
    # --max_frames N writes N frames
    assert vd.main(argv + ["--max_frames", "3"] + (["--render_as_pointcloud"] if pointcloud else [])) == 0
    assert np.array_equal(decoded(out), want[:3])
    assert not [f for f in os.listdir(os.path.dirname(out)) if "_tmp_" in f]


def test_a_fully_given_target_launches_no_centre_kernel(clip, monkeypatch):
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    paths, depth, color, Ts = clip

    def no_centres(*a, **k):
        raise AssertionError("the centres were computed although --tx --ty --tz are all given")
    monkeypatch.setattr(vd, "centers", no_centres)
    argv = ["--depth_video", paths["depth"], "--xfov", "45", "--render", "--tx", "0", "--ty", "0.1", "--tz", "4", "--x", "0.6", "--y", "0.5", "--z", "-1.2"]
    assert vd.main(argv) == 0                                        # (no --color_video: the depth video's bytes are the colour, 3dv:150)
    got = decoded(paths["depth"] + "_render.mkv")
    assert got.shape == (N, H, W, 3)
    with pytest.raises(AssertionError, match="centres were computed"):
        vd.main(argv[:-10] + ["--tx", "0", "--ty", "0.1"])           # tz left at -99.0: the centre is needed
