"""The geometry export's host side -- no GPU: the new header and its binding, tests/geometry_ref.py against the reference's own
arrays (tests/golden/geometry.npz, made by get_mesh_from_depth_map), the .ply / .obj files of geometry_files, the exporter tool's
refusals and frame bounds, and the condition the GPU test of the grey depth rests on."""
import importlib.util
import os
import re

import numpy as np
import pytest

import footprint as fp
import geometry_ref as gr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdvt_geometry.h")


def load_tool():
    spec = importlib.util.spec_from_file_location("export_depth_geometry", os.path.join(REPO, "tools", "export_depth_geometry.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(REPO, "tests", "golden", "geometry.npz"))


def test_the_header_parses_and_its_entry_points_are_bound():
    import ctypes as C
    from metric_depth_video_toolbox_amd import _lib
    decls = fp.header_entry_points(HEADER)
    assert sorted(decls) == sorted(_lib.GEOMETRY_SYMBOLS) == ["mdvt_depth_grey_batch", "mdvt_export_geometry_batch"]
    L = _lib.load()
    main_header = open(os.path.join(REPO, "include", "mdvt.h")).read()
    for name, args in decls.items():
        assert hasattr(L, name), f"{name} is not exported"
        assert name not in _lib.SYMBOLS and name not in main_header
        assert getattr(L, name).argtypes[-1] is C.c_void_p and name not in _lib.NO_STREAM
        assert re.search(r"void\s*\*\s*stream$", args), "only enqueues on the caller's stream"
        assert not re.search(r"\b(int|uint32_t|unsigned)\s+\w*(pitch|stride)\b", args), "pitches and strides are 64-bit"
    assert fp.takes_far_arguments(decls["mdvt_depth_grey_batch"]) and fp.writes_through_a_pointer(decls["mdvt_depth_grey_batch"])
    hdr = open(HEADER).read()
    struct = re.search(r"typedef struct mdvt_geometry_io \{(.*?)\} mdvt_geometry_io;", hdr, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", " ", struct, flags=re.S)
    assert len(re.findall(r"\bsize_t\s+\w+_(?:pitch|stride)\b", struct)) == 9 and not re.search(r"\b(int|uint32_t)\s+\w*(pitch|stride)", struct)
    for doc in ("cmf:692", "dmt:1378-1384", "dmt:1243-1254", "cmf:752-760", "Footprint:", "DECREE", "saturates", "MDVT_ERR_INVALID_ARG",
                "MDVT_ERR_UNSUPPORTED"):
        assert doc in hdr, doc
    assert C.sizeof(_lib.MdvtGeometryOpts) == 24 and C.sizeof(_lib.MdvtGeometryIO) == 17 * 8
    assert L.mdvt_version() == 15                                   # ABI 0.15: include/mdvt.h is unchanged


@pytest.mark.parametrize("scene", ["a", "b", "c"])
def test_geometry_ref_gives_the_references_own_arrays(gold, scene):
    rgb, K, max_depth = gold[f"{scene}_depth_rgb"], gold[f"{scene}_K"], float(gold[f"{scene}_max_depth"][0])
    H, W = rgb.shape[:2]
    assert gr.depth_of(rgb, 1, max_depth).tobytes() == gold[f"{scene}_depth"].tobytes()
    f = gr.export(rgb, K, decode=1, remove_edges=True, max_depth=max_depth, color_rgb=gold[f"{scene}_color"])
    assert f.vertices.dtype == np.float64 and f.vertices.tobytes() == gold[f"{scene}_pts_obo1"].tobytes()
    invalid = gold[f"{scene}_tri_invalid_obo1"]
    assert np.array_equal(f.tri_invalid != 0, invalid)
    # the reference's own arrays: triangles_all of dmt:1243-1254 without the flagged ones, and their vertices (dmt:1378-1384)
    want_tris = gr.topology(W, H)[~invalid]
    assert f.triangles.dtype == np.int32 and np.array_equal(f.triangles, want_tris)
    want_used = np.unique(want_tris.ravel())
    assert np.array_equal(f.used_index, want_used) and np.all(np.diff(f.used_index) > 0)
    assert f.counts == (len(want_used), len(want_tris)) and 0 < f.counts[1] < 2 * (H - 1) * (W - 1)
    # not the complement of the filter's unused list: a vertex may belong to a kept and to a removed triangle
    unused = gold[f"{scene}_unused_obo1"]
    assert np.intersect1d(unused, f.used_index).size > 0
    assert np.array_equal(f.points, gold[f"{scene}_pts_obo1"][want_used])
    assert np.array_equal(f.point_rgb, np.rint(gold[f"{scene}_colors_obo1"][want_used] * 255.0).astype(np.uint8))
    if scene == "b":                                                # the zero-depth patch: its triangles are removed, its inner vertices unused
        zero = np.flatnonzero(gold["b_depth"].ravel() == 0)
        assert zero.size > 4 and not np.isin(zero, f.used_index).all()
        cells = gr.topology(W, H)
        all_zero = np.isin(cells, zero).all(axis=1)
        assert all_zero.any() and invalid[all_zero].all()
    none = gr.export(rgb, K, decode=1, remove_edges=False, max_depth=max_depth)
    assert none.counts == (W * H, 2 * (H - 1) * (W - 1)) and np.array_equal(none.used_index, np.arange(W * H))


def test_the_exporters_decode_is_one_division(gold):
    rgb = gold["a_depth_rgb"].copy()
    rgb[..., 1] = rgb[..., 0] ^ 1                                    # R != G, an odd sum
    c = gr.codes(rgb, 0)
    assert np.array_equal(c >> 24, (rgb[..., 0].astype(np.uint32) + rgb[..., 1]) // 2) and np.array_equal((c >> 16) & 255, rgb[..., 2])
    # cmf:646-652 as written
    depth = np.zeros(rgb.shape[:2], np.uint32)
    unit = depth.view(np.uint8).reshape(rgb.shape[:2] + (4,))
    unit[..., 3] = ((rgb[..., 0].astype(np.uint32) + rgb[..., 1]).astype(np.uint32) / 2)
    unit[..., 2] = rgb[..., 2]
    want = depth.astype(np.float32) / ((255 ** 4) / 100)
    assert want.dtype == np.float32 and gr.depth_of(rgb, 0, 100).tobytes() == want.tobytes()
    assert np.any(gr.depth_of(rgb, 0, 100) != gr.depth_of(rgb, 1, 100))


@pytest.mark.parametrize("n", [0, 2, 5])
def test_ply_and_obj_round_trip_bit_for_bit(tmp_path, n):
    from metric_depth_video_toolbox_amd import geometry_files as gf
    rng = np.random.default_rng(n)
    pts = rng.normal(size=(n, 3)) * np.array([1e-9, 1.0, 1e12])
    if n:
        pts[0] = [0.1, -0.0, 1.0 / 3.0]
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    tris = np.array([[0, 1, 2], [2, 1, 4]], np.int32)[: (0 if n < 5 else 2)]
    gf.write_ply(tmp_path / "p.ply", pts, col)
    p, c = gf.read_ply(tmp_path / "p.ply")
    assert p.dtype == np.float64 and p.shape == (n, 3) and p.tobytes() == pts.tobytes() and np.array_equal(c, col) and c.dtype == np.uint8
    gf.write_obj(tmp_path / "m.obj", pts, col, tris)
    v, c, t = gf.read_obj(tmp_path / "m.obj")
    assert v.shape == (n, 3) and v.tobytes() == pts.tobytes() and np.array_equal(c, col) and np.array_equal(t, tris) and t.dtype == np.int32
    assert sorted(os.listdir(tmp_path)) == ["m.obj", "p.ply"], "no tmp file is left"


def test_the_files_bytes(tmp_path):
    import struct
    from metric_depth_video_toolbox_amd import geometry_files as gf
    gf.write_ply(tmp_path / "p.ply", np.array([[1.0, -2.0, 0.5], [0.0, 3.0, 4.0]]), np.array([[255, 0, 7], [1, 2, 3]], np.uint8))
    want = (b"ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex 2\nproperty double x\nproperty double y\n"
            b"property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
            + struct.pack("<3d3B", 1.0, -2.0, 0.5, 255, 0, 7) + struct.pack("<3d3B", 0.0, 3.0, 4.0, 1, 2, 3))
    assert open(tmp_path / "p.ply", "rb").read() == want
    gf.write_obj(tmp_path / "m.obj", np.array([[0.0, 0.0, 1.0], [1.5, 0.0, 1.0], [0.1, -2.0, 1e-7]]),
                 np.array([[255, 0, 0], [0, 255, 0], [51, 0, 255]], np.uint8), np.array([[0, 1, 2]], np.int32))
    want = (b"# Created by Open3D\n# number of vertices: 3\n# number of triangles: 1\n"
            b"v 0.0 0.0 1.0 1.0 0.0 0.0\nv 1.5 0.0 1.0 0.0 1.0 0.0\nv 0.1 -2.0 1e-07 0.2 0.0 1.0\nf 1 2 3\n")
    assert open(tmp_path / "m.obj", "rb").read() == want
    with pytest.raises(ValueError):
        gf.write_obj(tmp_path / "bad.obj", np.zeros((2, 3)), np.zeros((2, 3), np.uint8), np.array([[0, 1, 2]]))
    with pytest.raises(TypeError):
        gf.write_ply(tmp_path / "bad.ply", np.zeros((2, 3)), np.zeros((2, 3), np.float64))
    assert sorted(os.listdir(tmp_path)) == ["m.obj", "p.ply"]


def test_the_tool_refuses_what_is_not_built_before_a_file_is_opened(tmp_path):
    tool = load_tool()
    missing = str(tmp_path / "no_such_video.mkv")
    flags = {"track_file": ["--track_file", "t.json"], "mask_video": ["--mask_video", "m.mkv"], "strict_mask": ["--strict_mask"],
             "merge_close_points": ["--merge_close_points"], "save_alembic": ["--save_alembic"],
             "use_triangulated_points": ["--use_triangulated_points"], "save_rescaled_depth": ["--save_rescaled_depth"],
             "global_align": ["--global_align"], "show_scene_point_clouds": ["--show_scene_point_clouds"],
             "show_both_point_clouds": ["--show_both_point_clouds"]}
    assert sorted(flags) == sorted(tool.REFUSED)
    for name, argv in flags.items():
        with pytest.raises(NotImplementedError) as e:                # (the depth video does not exist: a refusal after opening would not be this error)
            tool.main(["--depth_video", missing, "--xfov", "60", "--save_ply", str(tmp_path / "ply")] + argv)
        assert str(e.value) == tool.REFUSED[name] and f"--{name}" in str(e.value)
    assert os.listdir(tmp_path) == []
    a = tool.build_parser().parse_args(["--depth_video", "x.mkv"])
    assert (a.min_frames, a.max_frames, a.max_depth, a.transformation_lock_frame, a.batch, a.video_decoder) == (-1, -1, 100, 0, 8, "host")
    tool.check_flags(a)
    helps = tool.build_parser().format_help()
    assert "min_frames + 1" in helps and "max_frames + 1" in helps and "16-bit grey" in helps


def test_the_frame_bounds_are_the_reference_loops():
    tool = load_tool()

    def loop(n, lo, hi):                                             # cmf:619-768 with everything but the counters taken out
        taken, frame_n = [], 0
        while frame_n < n:
            if lo >= frame_n and lo != -1:
                frame_n += 1
                continue
            taken.append(frame_n)
            if hi < frame_n and hi != -1:
                break
            frame_n += 1
        return taken

    assert tool.exported_frames(6) == [0, 1, 2, 3, 4, 5]
    assert tool.exported_frames(6, min_frames=1) == [2, 3, 4, 5], "frames 0 .. min_frames are skipped"
    assert tool.exported_frames(6, min_frames=0) == [1, 2, 3, 4, 5]
    assert tool.exported_frames(6, max_frames=2) == [0, 1, 2, 3], "the loop stops after frame max_frames + 1"
    assert tool.exported_frames(6, max_frames=0) == [0, 1]
    assert tool.exported_frames(10, min_frames=5, max_frames=2) == [6]
    for n in (0, 1, 7):
        for lo in range(-1, 9):
            for hi in range(-1, 9):
                assert tool.exported_frames(n, lo, hi) == loop(n, lo, hi), (n, lo, hi)
    assert list(tool._batches([2, 3, 4, 5, 6], 2)) == [[2, 3], [4, 5], [6]]


@pytest.mark.parametrize("max_depth", [100, 20])
def test_only_codes_above_the_encoders_maximum_leave_the_grey_range(max_depth):
    """All 65 536 (high, low) codes: where NumPy's value is beyond the type's range -- the set tests/test_gpu_geometry.py holds to
    saturation and not to NumPy's undefined cast -- the code is above 255^4."""
    hi, lo = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgb = np.stack([hi, hi, lo], axis=-1)
    code = gr.codes(rgb, 0).astype(np.int64)
    assert np.array_equal(code, (hi.astype(np.int64) << 24) | (lo.astype(np.int64) << 16))
    for bits in (16, 8):
        v, ok, out = gr.grey(rgb, max_depth, bits)
        assert v.dtype == np.float32 and (~ok).sum() > 0
        assert np.all(code[~ok] > gr.CODE_MAX), "a code the encoder can produce leaves the range"
        assert np.all(out[~ok] == (65535 if bits == 16 else 255))
        plain = np.rint(gr.depth_of(rgb, 0, max_depth) * ((255 ** 2 if bits == 16 else 255) / max_depth))[ok]
        assert np.array_equal(out[ok].reshape(plain.size, -1)[:, 0], plain.astype(out.dtype))
