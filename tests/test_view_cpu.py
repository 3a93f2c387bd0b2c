"""view_depthfile's host side -- no GPU: the reference's cam_look_at bit for bit (tests/golden/view_look_at.npz), the view matrix the
project renders with, the -99.0 sentinel and the float32 camera position of 3dv:231-239, the NumPy restatement of the centre
(tests/view_ref.py) against the reference's own vertices and their sequential mean, the order of np.sum in float64 restated in plain
Python (the order csrc/mdvt_view.hip reproduces: if a NumPy upgrade changes it, this test says so and not a GPU test), and the new
header."""
import os
import re

import numpy as np
import pytest

import footprint as fp
import view_ref as vr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the footprint of include/mdvt_view.h's entry points: what tests/test_gpu_view_centers.py holds them to
FOOTPRINT = {
    "mdvt_view_centers": dict(writes="3 * n_frames doubles of d_centers", reads="the first 3 W bytes of each depth row",
                              far="test_centers_of_frames_more_than_4_gib_apart", file="test_gpu_view_centers.py"),
    "mdvt_render_view_batch": dict(writes="the first 3 W bytes of each row of rgb, W of mask, 4 W of depth, n_frames words of hole_counts",
                                   reads="the first 3 W bytes of each depth and colour row",
                                   far="test_a_view_of_frames_more_than_4_gib_apart", file="test_gpu_view_render.py"),
}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(REPO, "tests", "golden", "view_look_at.npz"))


def test_the_header_parses_and_its_entry_points_are_bound():
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(os.path.join(REPO, "include", "mdvt_view.h"))
    assert sorted(decls) == sorted(_lib.VIEW_SYMBOLS) == sorted(FOOTPRINT)
    L = _lib.load()
    for name, args in decls.items():
        assert hasattr(L, name) and name not in _lib.SYMBOLS
        if name == "mdvt_view_centers":
            assert fp.takes_far_arguments(args) and fp.writes_through_a_pointer(args)
        assert re.search(r"void\s*\*\s*stream$", args), "only enqueues on the caller's stream"
        assert not re.search(r"\b(int|uint32_t|unsigned)\s+\w*(pitch|stride)\b", args), "pitches and strides are 64-bit"
        assert FOOTPRINT[name]["far"].startswith("test_")
        src = open(os.path.join(REPO, "tests", FOOTPRINT[name]["file"])).read()
        assert f"def {FOOTPRINT[name]['far']}(" in src
    hdr = open(os.path.join(REPO, "include", "mdvt_view.h")).read()
    for doc in ("3dv:231", "dmt:1091", "dmt:1112-1133", "DECREE", "MDVT_ERR_INVALID_ARG", "MDVT_ERR_UNSUPPORTED", "Footprint:", "8192"):
        assert doc in hdr, doc
    assert "mdvt_view_centers" not in open(os.path.join(REPO, "include", "mdvt.h")).read()
    assert L.mdvt_version() == 15                                   # ABI 0.15: include/mdvt.h is unchanged


def test_cam_look_at_is_the_references(gold):
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    pos, target, want = gold["look_pos"], gold["look_target"], gold["look_mat"]
    assert pos.dtype == np.float32 and len(pos) >= 5
    assert np.array_equal(pos[0], np.array(vd.DEFAULT_CAMERA, np.float32))          # the defaults of 3dv:42-44 are among them
    for p, t, w in zip(pos, target, want):
        got = vd.cam_look_at(p, t)
        assert got.dtype == np.float64 and got.tobytes() == w.tobytes(), (p, t, got - w)
    # what makes it no world-to-camera matrix: the position in the last column (z negated), a last row that is not (0, 0, 0, 1)
    m = vd.cam_look_at(pos[0], target[0])
    assert m[0, 3] == 2.0 and m[2, 3] == 4.0 and np.any(m[3, :3] != 0.0)


def test_look_at_view_is_a_rigid_world_to_camera_matrix():
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    assert np.array_equal(vd.look_at_view((0, 0, 0), (0, 0, 1)), np.eye(4))
    rng = np.random.default_rng(5)
    cases = [(vd.camera_position(), np.array([0.1, -0.2, 3.0]))] + [(rng.normal(size=3) * 5, rng.normal(size=3) * 5) for _ in range(20)]
    for p, t in cases:
        V = vd.look_at_view(p, t)
        R = V[:3, :3]
        assert V.dtype == np.float64 and np.array_equal(V[3], [0, 0, 0, 1])
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15
        assert np.linalg.det(R) > 0.999                              # x right, y down, z forward: a rotation, not a mirror
        d = np.linalg.norm(t - p)
        assert np.abs(V @ np.append(p, 1.0) - [0, 0, 0, 1]).max() <= 1e-14 * max(1.0, np.abs(p).max())
        assert np.abs(V @ np.append(t, 1.0) - [0, 0, d, 1]).max() <= 1e-14 * max(1.0, np.abs(p).max() + d)
    # y down: a point above the target (smaller y in this path's axes) has a negative camera y
    V = vd.look_at_view((0, 0, -4), (0, 0, 0))
    assert (V @ np.array([0, -1.0, 0, 1]))[1] < 0 and (V @ np.array([1.0, 0, 0, 1]))[0] > 0
    with pytest.raises(ValueError, match="stands on its target"):
        vd.look_at_view((1, 2, 3), (1, 2, 3))
    with pytest.raises(ValueError, match="above or below"):
        vd.look_at_view((1, 2, 3), (1, 5, 3))


def test_the_sentinel_and_the_float32_camera_position():
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    c = np.array([0.25, -0.5, 3.0])
    assert np.array_equal(vd.look_at_target(c), c)
    assert np.array_equal(vd.look_at_target(c, ty=1.5), [0.25, 1.5, 3.0])
    assert np.array_equal(vd.look_at_target(c, -99.0, 0.0, -99.0), [0.25, 0.0, 3.0])
    assert np.array_equal(vd.look_at_target(c, tx=-99.00001), [-99.00001, -0.5, 3.0])      # only an exact -99.0 is the sentinel
    assert vd.needs_center() and vd.needs_center(1.0, 2.0, -99.0) and not vd.needs_center(1.0, 2.0, 3.0)
    assert np.array_equal(vd.look_at_target(None, 1.0, 2.0, 3.0), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="centre"):
        vd.look_at_target(None, 1.0, -99.0, 3.0)
    p = vd.camera_position(0.1, 2.0, -4.7)
    assert p.dtype == np.float64
    assert p[0] == float(np.float32(0.1)) != 0.1 and p[2] == float(np.float32(-4.7)) and p[1] == 2.0
    assert np.array_equal(vd.camera_position(), [2.0, 2.0, -4.0])


def test_view_params_compose_the_view_with_the_pose():
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    from metric_depth_video_toolbox_amd.stereo_rerender import make_frame_params
    T = np.eye(4)
    T[:3, 3] = [0.1, -0.2, 0.3]
    posed = make_frame_params(64, 48, xfov=60.0, transformation=T, convergence_distance=2.0)
    plain = make_frame_params(64, 48, xfov=60.0)
    assert posed.convergence_angle != 0.0
    V = np.stack([vd.look_at_view(vd.camera_position(), (0, 0, 3)), vd.look_at_view((1, 0, 0), (0, 0.5, 2))])
    out = vd.view_params([posed, plain], V)
    got = [np.array([out[k].T[i] for i in range(16)]).reshape(4, 4) for k in range(2)]
    assert got[0].tobytes() == (V[0] @ T).tobytes() and got[1].tobytes() == (V[1] @ np.eye(4)).tobytes()
    assert [out[k].has_T for k in range(2)] == [1, 1] and out[0].convergence_angle == 0.0
    assert [out[0].K[i] for i in range(9)] == [posed.K[i] for i in range(9)] and out[0].depth_scale == posed.depth_scale
    assert posed.convergence_angle != 0.0 and plain.has_T == 0           # the inputs are copies' sources, not changed
    with pytest.raises(ValueError, match="2 frame parameter records"):
        vd.view_params([plain], V)


def _sum_in_numpys_order(a):
    """np.sum of a contiguous float64 array, in plain Python floats: chunks of the ufunc buffer, each pairwise, added in sequence."""
    def pw(a):
        n = len(a)
        if n < 8:
            r = 0.0
            for x in a:
                r = r + x
            return r
        if n <= 128:
            r = list(a[:8])
            i = 8
            while i < n - n % 8:
                for k in range(8):
                    r[k] = r[k] + a[i + k]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while i < n:
                res = res + a[i]
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return pw(a[:n2]) + pw(a[n2:])
    acc = 0.0
    for c in range(0, len(a), 8192):
        acc = acc + pw(a[c:c + 8192])
    return acc


@pytest.mark.parametrize("n", [1, 7, 16, 6144, 9250, 16512, 20000])
def test_numpy_sums_float64_in_chunks_of_8192_pairwise(n):
    assert np.getbufsize() == 8192
    rng = np.random.default_rng(n)
    P = rng.normal(size=(n, 3)) * rng.integers(1, 1000, (n, 1))
    for c in range(3):
        col = np.ascontiguousarray(P[:, c])
        assert float(np.sum(col)) == _sum_in_numpys_order([float(v) for v in col])
    assert vr.center_of(P).tobytes() == np.array([_sum_in_numpys_order([float(v) for v in P[:, c]]) / n for c in range(3)]).tobytes()


@pytest.mark.parametrize("mode", ["mesh", "points"])
def test_the_restated_centre_against_the_references_vertices(gold, mode):
    depth_rgb, K = gold["depth_rgb"], gold["K"]
    want_v, want_mean = gold["vertices_" + mode], gold["mean_" + mode]
    P = vr.vertices(depth_rgb, K, mesh=mode == "mesh", max_depth=float(gold["max_depth"]))
    assert P.dtype == np.float64 and P.tobytes() == want_v.tobytes()          # the vertex chain is the reference's, bit for bit
    # the reference's mean adds the rows one after the other: a sequential sum, as Open3D's get_center
    seq = np.zeros(3)
    for row in want_v:
        seq = seq + row
    assert (seq / len(want_v)).tobytes() == want_mean.tobytes()
    got, bound = vr.center_of(P), vr.center_bound(P)
    assert np.all(bound > 0) and np.all(bound < 1e-11)
    assert np.all(np.abs(got - want_mean) <= bound), (got - want_mean, bound)
    # a pose and the parking keep the bound: against the sequential sum of the same vertices
    T = np.array([[0.96, 0.0, 0.28, 0.1], [0.0, 1.0, 0.0, -0.2], [-0.28, 0.0, 0.96, 0.5], [0, 0, 0, 1.0]])
    Q = vr.vertices(depth_rgb, K, mesh=mode == "mesh", remove_edges=True, T=T)
    parked = np.all(Q == vr.PARKED, axis=1)
    assert parked.any() == (mode == "points") and not parked.all()
    seq = np.zeros(3)
    for row in Q:
        seq = seq + row
    assert np.all(np.abs(vr.center_of(Q) - seq / len(Q)) <= vr.center_bound(Q))


def test_every_refused_flag_raises_and_names_its_reason(tmp_path):
    from metric_depth_video_toolbox_amd import view_depthfile as vd
    d = str(tmp_path / "d.npy")
    np.save(d, np.zeros((2, 4, 4, 3), np.uint8))
    base = ["--depth_video", d, "--xfov", "45"]
    cases = [([], "interactive window"), (["--render", "--draw_frame", "1"], "GUI"), (["--render", "--show_camera"], "LineSet"),
             (["--render", "--background_ply", "x.ply"], "point cloud"), (["--render", "--compressed"], "FFV1"),
             (["--render", "--mask_video", "m.mkv"], "dmt:1326-1334"), (["--render", "--invert_mask"], "dmt:1326-1334")]
    for extra, reason in cases:
        with pytest.raises(NotImplementedError, match=reason):
            vd.main(base + extra)
    a = vd.build_parser().parse_args(base + ["--render"])
    assert (a.x, a.y, a.z, a.tx, a.ty, a.tz) == (2.0, 2.0, -4.0, -99.0, -99.0, -99.0)
    assert (a.max_depth, a.max_frames, a.transformation_lock_frame, a.batch, a.video_decoder, a.video_encoder) == (100, -1, 0, 8, "host", "host")
    assert not a.render_as_pointcloud and not a.remove_edges and a.color_video is None and a.transformation_file is None
    with pytest.raises(ValueError, match="--xfov or --yfov"):
        vd.main(["--depth_video", d, "--render"])
    with pytest.raises(Exception, match="does not exist"):
        vd.main(["--depth_video", str(tmp_path / "no.npy"), "--xfov", "45", "--render"])
    assert sorted(os.listdir(tmp_path)) == ["d.npy"]                 # refused before anything was written
