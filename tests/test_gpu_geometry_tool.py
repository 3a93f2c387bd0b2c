"""tools/export_depth_geometry.py end to end on a 4-frame 24 x 16 .mkv pair with a transformation file and a lock frame: the .ply and
.obj files read back with geometry_files equal tests/geometry_ref.py, --bit8 decodes to the grey reference and the --bit16 dump
equals it, the host and the device decoder give the same files, the frame bounds are the reference loop's, no tmp file is left."""
import importlib.util
import json
import os

import numpy as np
import pytest

import geometry_cases as gc
import geometry_ref as gr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 24, 16, 4


@pytest.fixture(scope="module")
def tool():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    spec = importlib.util.spec_from_file_location("export_depth_geometry", os.path.join(REPO, "tools", "export_depth_geometry.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """The files and the reference of every frame -- computed once."""
    from metric_depth_video_toolbox_amd import depth_map_tools, distributed, video_io
    d = tmp_path_factory.mktemp("geometry_tool")
    rng = np.random.default_rng(24)
    depth = np.stack([gc.scene(rng, H, W, f, split=True) for f in range(N)])
    color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    for name, frames in (("depth.mkv", depth), ("color.mkv", color)):
        with video_io.VideoWriter(str(d / name), W, H, 24.0) as w:
            for f in frames:
                w.write(np.ascontiguousarray(f))
    Ts = [np.eye(4)] + gc.poses(N)[1:]
    with open(d / "transforms.json", "w") as fh:
        json.dump([T.tolist() for T in Ts], fh)
    K = depth_map_tools.compute_camera_matrix(60.0, None, W, H)
    based = distributed.rebase_on_lock_frame(json.load(open(d / "transforms.json")), 2)        # cmf:599-603
    refs = [gr.export(depth[f], K, decode=0, remove_edges=1, T=based[f], color_rgb=color[f]) for f in range(N)]
    assert len({r.counts for r in refs}) > 1 and all(0 < r.counts[1] < 2 * (W - 1) * (H - 1) for r in refs)
    return dict(dir=d, depth=depth, color=color, refs=refs)


def run_tool(tool, clip, out, *extra):
    argv = ["--depth_video", str(clip["dir"] / "depth.mkv"), "--color_video", str(clip["dir"] / "color.mkv"), "--xfov", "60", "--remove_edges",
            "--transformation_file", str(clip["dir"] / "transforms.json"), "--transformation_lock_frame", "2", "--batch", "3",
            "--save_ply", str(out / "ply"), "--save_obj", str(out / "obj")] + list(extra)
    assert tool.main(argv) == 0


def check_files(clip, out, frames):
    from metric_depth_video_toolbox_amd import geometry_files as gf
    assert sorted(os.listdir(out / "ply")) == [f"{f:07d}.ply" for f in frames], "file names, frame bounds, no tmp file"
    assert sorted(os.listdir(out / "obj")) == [f"{f:07d}.obj" for f in frames]
    for f in frames:
        ref = clip["refs"][f]
        p, c = gf.read_ply(out / "ply" / f"{f:07d}.ply")
        assert p.tobytes() == ref.points.tobytes() and np.array_equal(c, ref.point_rgb), f"frame {f}: point cloud"
        v, c, t = gf.read_obj(out / "obj" / f"{f:07d}.obj")
        assert v.tobytes() == ref.vertices.tobytes() and np.array_equal(t, ref.triangles), f"frame {f}: mesh"
        assert np.array_equal(c, clip["color"][f].reshape(-1, 3))


def test_the_tool_writes_the_references_geometry_and_grey_depth(tool, clip, tmp_path):
    from metric_depth_video_toolbox_amd import clip_io
    host, dev = tmp_path / "host", tmp_path / "device"
    grey8 = str(clip["dir"] / "depth.mkv") + "_grey_depth.mkv"
    grey16 = str(clip["dir"] / "depth.mkv") + "_grey_depth.npy"
    run_tool(tool, clip, host, "--bit8")
    check_files(clip, host, range(N))
    frames = clip_io.open_frames(grey8, Exception("no grey video"))
    got = np.array(frames[0:N])
    for p, _ in clip_io.video_parts(frames):
        p.close()
    want8 = np.stack([gr.grey(clip["depth"][f], 100, 8)[2] for f in range(N)])
    assert got.shape == want8.shape and np.array_equal(got, want8)
    os.remove(grey8)
    run_tool(tool, clip, dev, "--bit16", "--video_decoder", "device")
    check_files(clip, dev, range(N))
    want16 = np.stack([gr.grey(clip["depth"][f], 100, 16)[2] for f in range(N)])
    got = np.load(grey16)
    assert got.dtype == np.uint16 and np.array_equal(got, want16)
    os.remove(grey16)
    for sub in ("ply", "obj"):                                       # the host and the device decoder: the same files
        for name in sorted(os.listdir(host / sub)):
            assert open(host / sub / name, "rb").read() == open(dev / sub / name, "rb").read(), name
    assert sorted(os.listdir(clip["dir"])) == ["color.mkv", "depth.mkv", "transforms.json"], "no tmp file is left"


def test_the_tools_frame_bounds(tool, clip, tmp_path):
    run_tool(tool, clip, tmp_path, "--min_frames", "0", "--max_frames", "1")
    assert tool.exported_frames(N, 0, 1) == [1, 2]
    check_files(clip, tmp_path, [1, 2])
