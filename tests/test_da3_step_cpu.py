"""The Depth-Anything-3 depth step's host side -- no GPU: the new header and its binding, the batch schedule against a plain loop, the
similarity fit and the last-frame correction of the poses, the four refusals, the parser's defaults and the file names with their
tmp -> rename step."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import depth_sink_ref as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdvt_depth_sink.h")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("video_da3_tool", os.path.join(REPO, "tools", "video_da3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def host():
    from metric_depth_video_toolbox_amd import video_da3
    return video_da3


def test_the_entry_point_is_exported_by_both_libraries_outside_the_main_header():
    import ctypes
    from metric_depth_video_toolbox_amd import _lib
    hdr = open(HEADER).read()
    declared = sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert declared == sorted(_lib.DEPTH_SINK_SYMBOLS) == ["mdvt_depth_video_codes"]
    L = _lib.load()
    for s in _lib.DEPTH_SINK_SYMBOLS:
        assert hasattr(L, s) and s not in _lib.SYMBOLS and s not in _lib.METRIC_ALIGN_SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.lib_path("tuning")), s)
        assert L.mdvt_depth_video_codes.argtypes[-1] is ctypes.c_void_p and len(L.mdvt_depth_video_codes.argtypes) == 20
    assert "mdvt_depth_video_codes" not in open(os.path.join(REPO, "include", "mdvt.h")).read()
    assert L.mdvt_version() == 15                                   # include/mdvt.h is unchanged
    decl = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    assert re.search(r"int mdvt_depth_video_codes\(mdvt_ctx\* ctx, int in_w, int in_h, int n_frames, const float\* d_depth, size_t depth_pitch, "
                     r"size_t depth_stride, const float\* d_scale, int nan_to_max, double max_depth, int out_w, int out_h, uint8_t\* d_codes, "
                     r"size_t codes_pitch, size_t codes_stride, int order, float\* d_plane, size_t plane_pitch, size_t plane_stride, "
                     r"void\* stream\);", decl)


def test_a_null_context_is_refused_without_a_device():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert L.mdvt_depth_video_codes(None, 4, 4, 1, None, 16, 64, None, 0, 100.0, 4, 4, None, 12, 48, 0, None, 16, 64, None) == -1


SCHEDULE_CASES = [(n, refs, overlap, batch) for n in range(1, 61) for refs in (0, 1, 6, 7) for overlap in (0, 1, 6) for batch in (1, 5, 40)]


def test_batch_schedule_equals_the_plain_loop(host):
    for n, refs, overlap, batch in SCHEDULE_CASES + [(100, 6, 6, 40)]:
        got = host.batch_schedule(n, batch, overlap, refs)
        want = dr.schedule(n, batch, overlap, refs)
        assert [(list(i), u) for i, u in got] == want, (n, refs, overlap, batch)
        new = [f for ids, used in got for f in ids[used:]]
        assert new == list(range(n))                                # every frame is written once, in order
    assert any(n < refs for n, refs, _, _ in SCHEDULE_CASES) and any(o >= b for _, _, o, b in SCHEDULE_CASES)


def test_the_schedules_quirks(host):
    assert host.reference_frame_ids(100, 6) == [0, 16, 32, 48, 64, 80, 96]                     # 7 references for 6
    assert host.reference_frame_ids(5, 6) == [0] and host.reference_frame_ids(5, 0) == []
    s = host.batch_schedule(12, 5, 0, 1)                                                       # references 0 .. 11: nth = 12
    assert s[1] == ([0] + [0, 1, 2, 3, 4] + [5, 6, 7, 8, 9], 6)                                # an overlap of 0 hands over the whole batch
    s = host.batch_schedule(100, 40, 6, 6)
    assert [len(ids) for ids, _ in s] == [7 + 40, 7 + 6 + 40, 7 + 6 + 20] and [u for _, u in s] == [7, 13, 13]      # vd3:141 is never used
    s = host.batch_schedule(7, 1, 6, 0)                                                        # overlap >= batch: the one frame there is
    assert s[3] == ([2, 3], 1)
    with pytest.raises(ValueError):
        host.batch_schedule(5, 0, 1, 1)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _poses(rng, n):
    out = []
    for _ in range(n):
        R = _rotation(rng)
        out.append(np.hstack([R, rng.normal(size=(3, 1))]))
    return np.stack(out)


@pytest.mark.parametrize("n", [3, 4, 9])
def test_the_sim3_fit_recovers_a_known_similarity(host, n):
    rng = np.random.default_rng(n)
    src = rng.normal(size=(n, 3))
    s, R, t = 0.37 + n, _rotation(rng), rng.normal(size=3)
    dst = s * src @ R.T + t
    gs, gR, gt = host.sim3_from_centres(src, dst)
    assert abs(gs - s) < 1e-9 and np.abs(gR - R).max() < 1e-9 and np.abs(gt - t).max() < 1e-9
    ws, wR, wt = dr.umeyama(src, dst)
    assert abs(gs - ws) < 1e-9 and np.abs(gR - wR).max() < 1e-9 and np.abs(gt - wt).max() < 1e-9
    # applied to poses: the centres move by the similarity, the rotations by R^T on the right
    poses = _poses(rng, 5)
    moved = host.apply_sim3(poses, s, R, t)
    assert np.abs(host.camera_centres(moved) - (s * host.camera_centres(poses) @ R.T + t)).max() < 1e-9
    assert np.abs(moved[:, :, :3] - poses[:, :, :3] @ R.T).max() < 1e-12
    assert np.abs(moved - dr.apply_sim3(poses, s, R, t)).max() < 1e-12


def test_the_sim3_fit_is_the_identity_where_it_is_undefined(host):
    rng = np.random.default_rng(2)
    for src, dst in ((rng.normal(size=(2, 3)), rng.normal(size=(2, 3))),                       # 2 poses
                     (np.tile(rng.normal(size=(1, 3)), (4, 1)), rng.normal(size=(4, 3))),      # coincident centres
                     (np.full((3, 3), np.nan), rng.normal(size=(3, 3)))):
        s, R, t = host.sim3_from_centres(src, dst)
        assert s == 1.0 and np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))


def test_the_last_frame_correction_maps_the_last_reference_pose_onto_the_earlier_one(host):
    rng = np.random.default_rng(5)
    earlier, refs, new = _poses(rng, 5), _poses(rng, 5), _poses(rng, 4)
    diff = host.last_frame_correction(earlier[-1], refs[-1])
    assert np.abs(diff @ host.pose4(refs[-1]) - host.pose4(earlier[-1])).max() < 1e-13
    # the whole alignment: a batch that is the earlier one re-gauged by a rigid transform comes back exactly
    G = np.vstack([np.hstack([_rotation(rng), rng.normal(size=(3, 1))]), [0, 0, 0, 1]])
    regauged = np.stack([(host.pose4(p) @ G)[:3] for p in np.concatenate([earlier, new])])
    got = host.align_batch_poses(earlier, regauged[:5], regauged[5:])
    assert np.abs(got - new).max() < 1e-9
    # two reference poses only: no similarity, the correction alone still lands the last one
    got = host.align_batch_poses(earlier[:2], regauged[:2], regauged[1:2])
    assert np.abs(got[0] - earlier[1]).max() < 1e-12


@pytest.mark.parametrize("flag,value", [("--xfov", "60"), ("--yfov", "40"), ("--xfov_file", "fovs.json"), ("--transformation_file", "t.json")])
def test_the_four_refused_flags_raise_before_a_file_is_opened(host, tool, tmp_path, flag, value):
    missing = str(tmp_path / "no_such_clip.mkv")                    # were a file opened, this would fail first, with another error
    args = host.build_parser().parse_args(["--color_video", missing, flag, value, "--generator", "no.such.module:fn"])
    with pytest.raises(NotImplementedError, match=r"video_da3\.py:(102|112)"):
        tool.run(args)
    assert os.listdir(tmp_path) == []


def test_the_parsers_defaults_are_the_references(host):
    a = host.build_parser().parse_args(["--color_video", "x.mkv"])
    assert (a.max_frames, a.max_depth, a.images_per_batch, a.batch_overlap, a.nr_of_ref_frames, a.da3_resolution) == (-1, 100, 40, 6, 6, 504)
    assert a.xfov is None and a.yfov is None and a.xfov_file is None and a.transformation_file is None
    assert (a.generator, a.video_decoder, a.video_encoder) == ("da3", "host", "host")
    assert isinstance(host.build_parser().parse_args(["--color_video", "x", "--max_depth", "20"]).max_depth, int)


def test_the_default_generator_fails_with_one_line_where_da3_is_missing(host, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "depth_anything_3", None)      # (an import of it raises ImportError, installed or not)
    monkeypatch.setitem(sys.modules, "depth_anything_3.api", None)
    with pytest.raises(RuntimeError, match="depth_anything_3") as e:
        host.load_generator("da3")
    assert "\n" not in str(e.value)
    with pytest.raises(ValueError):
        host.load_generator("not_a_spec")


def test_file_names_and_the_tmp_rename_step(host, tmp_path):
    assert host.output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_xfovs.json",
                                          "x.mkv_depth.mkv_transformations.json")
    assert host.output_paths("x.npy", video=False)[:2] == ("x.npy_tmp_depth.npy", "x.npy_depth.npy")
    lst = tmp_path / "clips.txt"
    lst.write_text("# a list\n\n a.mkv \nb.mkv\n")
    assert host.clips_from_argument(str(lst)) == ["a.mkv", "b.mkv"] and host.clips_from_argument("a.mkv") == ["a.mkv"]
    # tmp -> final: the frames are written as tmp and renamed when their count is right; a failure leaves neither
    from metric_depth_video_toolbox_amd.clip_io import ClipOutput
    tmp, final, xf, tf = host.output_paths(str(tmp_path / "c.npy"), video=False)
    with ClipOutput(tmp, final, 2, (2, 3, 3)) as out:
        assert os.path.exists(tmp) and not os.path.exists(final)
        out.arr[...] = 7
    assert os.path.exists(final) and not os.path.exists(tmp) and np.load(final).shape == (2, 2, 3, 3)
    os.remove(final)
    with pytest.raises(KeyError):
        with ClipOutput(tmp, final, 2, (2, 3, 3)):
            raise KeyError("the batch loop failed")
    assert not os.path.exists(tmp) and not os.path.exists(final)
    T = [np.eye(4), np.arange(16.0).reshape(4, 4)]
    host.write_json_files(xf, tf, [np.float32(45.5), 60.0], T)
    assert json.load(open(xf)) == [45.5, 60.0] and json.load(open(tf)) == [t.tolist() for t in T]


def test_the_pose_track_writes_inverted_matrices_and_the_x_field_of_view(host):
    from metric_depth_video_toolbox_amd import depth_map_tools
    rng = np.random.default_rng(9)
    ext = _poses(rng, 4).astype(np.float32)
    K = np.stack([depth_map_tools.compute_camera_matrix(40.0 + k, None, 48, 32) for k in range(4)]).astype(np.float32)
    track = host.PoseTrack(2)
    track.add(ext, K, 1)                                            # one leading reference: three new frames
    assert len(track.extrinsics) == 3 and len(track.last) == 2
    for got, e in zip(track.transformations(), ext[1:]):
        assert np.abs(got @ host.pose4(e) - np.eye(4)).max() < 1e-6
    assert track.xfovs() == [float(depth_map_tools.fov_from_camera_matrix(k)[0]) for k in K[1:]]
    assert all(abs(f - (41.0 + k)) < 1e-4 for k, f in enumerate(track.xfovs()))
