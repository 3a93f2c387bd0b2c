"""Scene detection without a GPU: the HSV restatement of tests/scene_ref.py over every colour, the two detectors of
metric_depth_video_toolbox_amd/scene_detect.py on hand-made score series (and against the restatement), the CSV text, the header's
declaration and the host predicate of the 16-byte path."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import scene_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from metric_depth_video_toolbox_amd import scene_detect as sd      # noqa: E402


def test_the_host_module_needs_no_torch():
    import subprocess
    code = "import sys; import metric_depth_video_toolbox_amd.scene_detect; assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


# ---- HSV ------------------------------------------------------------------------------------------------------------------------
def test_hsv_over_all_colours():
    """V exact; S within 1 of 255 d / v; H within 1 (mod 180) of 30 h / d: the tables are rounded to integers (error <= 0.5, times at
    most 1530 / 4096 for H, 255 / 4096 for S), then the product is rounded (0.5): below 1 in both cases.  Derived, not measured."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r0 in range(0, 256, 16):
        rgb = np.empty((16, 256, 256, 3), np.uint8)
        rgb[..., 0] = np.arange(r0, r0 + 16)[:, None, None]
        rgb[..., 1] = g
        rgb[..., 2] = b
        H, S, V = sr.hsv_u8(rgb)
        c = rgb.astype(np.float64)
        R, G, B = c[..., 0], c[..., 1], c[..., 2]
        v = np.maximum(R, np.maximum(G, B))
        d = v - np.minimum(R, np.minimum(G, B))
        assert (V == v).all()
        assert H.min() >= 0 and H.max() < 180 and S.min() >= 0 and S.max() <= 255
        grey = d == 0
        assert (H[grey] == 0).all() and (S[grey] == 0).all()
        ok = ~grey
        assert (np.abs(S[ok] - 255.0 * d[ok] / v[ok]) <= 1.0).all()
        h = np.where(v == R, G - B, np.where(v == G, B - R + 2 * d, R - G + 4 * d))
        ideal = np.mod(30.0 * h[ok] / d[ok], 180.0)
        err = np.abs(H[ok] - ideal)
        assert (np.minimum(err, 180.0 - err) <= 1.0).all()


def test_hsv_ties_take_the_stated_branch():
    # v == r == g: the first branch (h = g - b = d -> H = 30), not the second (h = b - r + 2 d = d as well: the same hue, by continuity)
    H, S, V = sr.hsv_u8(np.array([[200, 200, 50]], np.uint8))
    assert (int(H[0]), int(V[0])) == (30, 200)
    # v == g == b: the second branch (h = b - r + 2 d = 3 d -> H = 90), not the third (r - g + 4 d = 3 d)
    H, S, V = sr.hsv_u8(np.array([[10, 180, 180]], np.uint8))
    assert int(H[0]) == 90
    # v == r == b: the first branch, h = g - b = -d -> H = -30 + 180 = 150 (the negative hue's wrap)
    H, S, V = sr.hsv_u8(np.array([[220, 20, 220]], np.uint8))
    assert int(H[0]) == 150
    # the six saturated primaries and secondaries
    prim = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]], np.uint8)
    H, S, V = sr.hsv_u8(prim)
    assert H.tolist() == [0, 30, 60, 90, 120, 150] and S.tolist() == [255] * 6 and V.tolist() == [255] * 6


def test_tables_round_ties_to_even():
    assert sr.SDIV[1] == 255 << 12 and sr.SDIV[0] == 0 and sr.HDIV[0] == 0 and sr.HDIV[1] == 122880
    for i in range(1, 256):                              # the integer form the kernel builds its tables with
        for n, tab in ((255 << 12, sr.SDIV), ((180 << 12) // 6, sr.HDIV)):
            q, r = divmod(n, i)
            want = q + 1 if 2 * r > i else (q + (q & 1) if 2 * r == i else q)
            assert tab[i] == want, (n, i)


def test_frame_sums_restatement_on_small_cases():
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (3, 6, 36, 3), dtype=np.uint8)
    assert sr.frame_sums(np.stack([f[0], f[0]])) == [[0, 0, 0]]
    a = sr.frame_sums(f)
    assert len(a) == 2 and sr.frame_sums(f[1:], prev=f[0]) == a
    assert sr.frame_sums(f[..., ::-1], bgr=True) == a
    white = np.full((1, 4, 8, 3), 255, np.uint8)
    assert sr.frame_sums(white, prev=np.zeros((4, 8, 3), np.uint8)) == [[0, 0, 255 * 32]]
    assert sr.analysed(f[0], 2).shape == (3, 18, 3) and sr.analysed_size(5, 2) == 2 and sr.analysed_size(7, 2) == 4


# ---- the detectors --------------------------------------------------------------------------------------------------------------
def _series(n, spikes, low=1.0):
    s = [low] * (n - 1)                                  # s[k - 1] is frame k's score
    for k, v in spikes.items():
        s[k - 1] = v
    return s


def test_content_cut_exactly_at_min_scene_len():
    assert sd.content_cuts(_series(40, {15: 30.0})) == [15]
    assert sd.content_cuts(_series(40, {14: 30.0})) == []
    assert sd.content_cuts(_series(40, {14: 30.0, 15: 27.0})) == [15]            # >= threshold
    assert sd.content_cuts(_series(40, {15: 26.999})) == []
    assert sd.content_cuts(_series(60, {15: 30.0, 29: 30.0, 30: 30.0})) == [15, 30]
    assert sd.content_cuts(_series(40, {3: 90.0}), min_scene_len=3) == [3]


def test_adaptive_rules():
    assert sd.adaptive_cuts(_series(40, {15: 30.0})) == [15]
    assert sd.adaptive_cuts(_series(40, {14: 30.0})) == []
    assert sd.adaptive_cuts(_series(40, {20: 14.9})) == []                       # ratio 14.9 but below min_content_val
    assert sd.adaptive_cuts(_series(40, {20: 30.0}, low=10.1)) == []             # ratio below 3
    assert sd.adaptive_cuts(_series(40, {20: 30.0}, low=10.0)) == [20]           # ratio exactly 3
    # the zero-average branch: identical frames around the spike
    assert sd.adaptive_cuts(_series(40, {20: 15.0}, low=0.0)) == [20]
    assert sd.adaptive_cuts(_series(40, {20: 14.0}, low=0.0)) == []
    # the first and the last two frames never cut (frame 0 has no score; 1, 2, n - 2, n - 1 lack a neighbour)
    for k in (1, 2, 38, 39):
        assert sd.adaptive_cuts(_series(40, {k: 200.0}), min_scene_len=0) == []
    assert sd.adaptive_cuts(_series(40, {3: 200.0}), min_scene_len=0) == [3]
    assert sd.adaptive_cuts(_series(40, {37: 200.0}), min_scene_len=0) == [37]
    assert sd.adaptive_cuts([50.0, 50.0, 50.0]) == []                            # too short for a window


def test_a_series_without_a_cut_is_one_scene():
    assert sd.scenes_from_cuts(sd.detect_cuts(_series(40, {}), "adaptive"), 40) == [(0, 40)]
    assert sd.scenes_from_cuts(sd.detect_cuts(_series(40, {}), "content"), 40) == [(0, 40)]
    assert sd.scenes_from_cuts([16, 32], 40) == [(0, 16), (16, 32), (32, 40)]
    with pytest.raises(ValueError, match="detector"):
        sd.detect_cuts([1.0], "edges")


def test_detectors_equal_the_restatement_on_random_series():
    rng = np.random.default_rng(11)
    for _ in range(50):
        s = list(rng.choice([0.0, 1.0, 5.0, 16.0, 30.0, 90.0], size=int(rng.integers(1, 80)), p=[.2, .4, .2, .1, .05, .05]))
        assert sd.content_cuts(s) == sr.content_cuts(s)
        assert sd.adaptive_cuts(s) == sr.adaptive_cuts(s)
    sums = [(3, 5, 7), (1 << 33, 2, 1)]
    assert sd.scores_from_sums(sums, 77) == sr.scores(sums, 77)


def test_downscale():
    assert [sd.auto_downscale(w) for w in (48, 255, 256, 511, 512, 1920)] == [1, 1, 1, 1, 2, 7]
    assert sd.downscale_factor("auto", 512, 8) == 2 and sd.downscale_factor("3", 70, 21) == 3
    assert sd.analysed_pixels(70, 21, 7) == 10 * 3 and sd.analysed_pixels(5, 7, 2) == 2 * 4      # round(2.5) = 2, round(3.5) = 4
    for n in range(1, 60):
        for f in range(1, 12):
            assert sd.round_half_even_div(n, f) == round(n / f) == sr.analysed_size(n, f)
    with pytest.raises(ValueError, match="leaves no image"):
        sd.downscale_factor(65, 48, 32)                   # 32 / 65 rounds to 0 rows
    with pytest.raises(ValueError, match=">= 1"):
        sd.downscale_factor(0, 48, 32)


# ---- the CSV ---------------------------------------------------------------------------------------------------------------------
CSV_TEXT = """Timecode List:,00:00:00.667,00:00:01.333
Scene Number,Start Frame,Start Timecode,Start Time (seconds),End Frame,End Timecode,End Time (seconds),Length (frames),Length (timecode),Length (seconds)
1,1,00:00:00.000,0.000,16,00:00:00.667,0.667,16,00:00:00.667,0.667
2,17,00:00:00.667,0.667,32,00:00:01.333,1.333,16,00:00:00.667,0.667
3,33,00:00:01.333,1.333,40,00:00:01.667,1.667,8,00:00:00.333,0.333
"""


def test_csv_text_byte_for_byte(tmp_path):
    scenes = [(0, 16), (16, 32), (32, 40)]
    assert sd.scene_csv_text(scenes, 24.0) == CSV_TEXT == sr.csv_text(scenes, 24.0)
    assert sd.scene_csv_text([(0, 90000)], 25.0).splitlines()[0] == "Timecode List:"
    assert sd.scene_csv_text([(0, 90000)], 25.0).splitlines()[2] == "1,1,00:00:00.000,0.000,90000,01:00:00.000,3600.000,90000,01:00:00.000,3600.000"
    path = str(tmp_path / "movie-Scenes.csv")
    assert sd.write_scene_csv(path, scenes, 24.0) == path
    assert open(path, newline="").read() == CSV_TEXT and os.listdir(tmp_path) == ["movie-Scenes.csv"]


def test_load_returns_what_was_written(tmp_path):
    scenes = [(0, 16), (16, 32), (32, 40)]
    for delim in (",", ";"):
        path = str(tmp_path / f"x{ord(delim)}.csv")
        sd.write_scene_csv(path, scenes, 23.976, delimiter=delim)
        rows = sd.load_scene_csv(path, delim)
        assert rows == sd.scene_rows(scenes, 23.976) and sd.scenes_of_rows(rows) == scenes
        assert list(rows[0]) == sd.CSV_HEADER
    assert sd.scene_file_path("/a/b/movie.part.mkv", "out") == os.path.join("out", "movie.part-Scenes.csv")


def test_flags_are_refused_before_anything_is_opened(tmp_path):
    p = sd.build_parser()
    for bad, text in ((["--batch", "0"], "batch"), (["--downscale", "0"], "downscale"), (["--fps", "0"], "fps"), (["--min_scene_len", "-1"], "min_scene_len")):
        with pytest.raises(ValueError, match=text):
            sd.check_flags(p.parse_args(["--color_video", str(tmp_path / "none.mkv")] + bad))
    sd.check_flags(p.parse_args(["--color_video", "x.mkv"]))
    assert p.parse_args(["--color_video", "x.mkv"]).detector == "adaptive"


# ---- the header and the library --------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_point_in_the_usual_form():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "mdvt_scene.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mdvt_scene_frame_sums\s*\(\s*mdvt_ctx\s*\*\s*ctx\s*,([^;]*)void\s*\*\s*stream\s*\)\s*;", text)
    assert m, "int mdvt_scene_frame_sums(mdvt_ctx* ctx, ..., void* stream);"
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",") if a.strip()]
    assert names == ["width", "height", "n_frames", "d_frames", "pitch", "stride", "order", "d_prev", "prev_pitch", "factor", "d_sums"]
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    assert len(L.mdvt_scene_frame_sums.argtypes) == len(names) + 2 and L.mdvt_scene_frame_sums.argtypes[-1] is C.c_void_p
    assert set(_lib.SCENE_SYMBOLS) == {"mdvt_scene_frame_sums", "mdvt_scene_vector_path"}


def test_the_vector_path_predicate():
    from metric_depth_video_toolbox_amd import _lib
    vec = _lib.load().mdvt_scene_vector_path
    assert vec(5, 4096, 192, 192 * 16, None, 0, 1) == 1
    assert vec(5, 4096, 192, 192 * 16, 8192, 208, 1) == 1
    assert vec(5, 4096, 192, 192 * 16, 8192, 208, 2) == 0         # a factor: the resize gathers bytes
    assert vec(5, 4097, 192, 192 * 16, None, 0, 1) == 0           # an odd base
    assert vec(5, 4096, 200, 200 * 16, None, 0, 1) == 0           # a pitch that is no multiple of 16
    assert vec(5, 4096, 192, 192 * 16 + 8, None, 0, 1) == 0       # a stride that is none
    assert vec(1, 4096, 192, 7, 8192, 192, 1) == 1                # one frame: the stride is not used
    assert vec(5, 4096, 192, 192 * 16, 8200, 192, 1) == 0 and vec(5, 4096, 192, 192 * 16, 8192, 200, 1) == 0


# ---- the driver's plan (metric_depth_video_toolbox_amd/movie_2_3D.py) ---------------------------------------------------------------
import copy      # noqa: E402
import importlib.util      # noqa: E402
import json      # noqa: E402

from metric_depth_video_toolbox_amd import movie_2_3D as m23      # noqa: E402


def _fixture():
    with open(os.path.join(REPO, "tests", "golden", "movie_scenes.json")) as fh:
        return json.load(fh)


def test_the_driver_module_needs_no_torch():
    import subprocess
    code = "import sys; import metric_depth_video_toolbox_amd.movie_2_3D; assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


def test_split_and_plan_equal_the_references_own_functions(tmp_path, monkeypatch):
    cases = _fixture()
    names = {c["name"] for c in cases}
    assert {"plain", "long_zero_extra", "long_end_scene", "columns"} <= names
    long = next(c for c in cases if c["name"] == "long_zero_extra")
    assert [s["Length (frames)"] for s in long["split"]] == ["100", "1500", "1500", "100", "0", "1500"]      # 3 100 frames at 1500, a scene of none
    assert long["split"][1]["Engine"] == "vda" and long["split"][5]["Note"] == "kept"
    monkeypatch.chdir(tmp_path)
    for c in cases:
        split = m23.split_scenes(copy.deepcopy(c["scenes"]), c["max_scene_frames"])
        assert split == c["split"], c["name"]
        out = "out"
        os.makedirs(out, exist_ok=True)
        for f in os.listdir(out):
            os.remove(os.path.join(out, f))
        for f in c["existing"]:
            open(os.path.join(out, f), "w").close()
        assert m23.plan_scene_files(copy.deepcopy(split), out, c["end_scene"]) == c["planned"], c["name"]
    ended = next(c for c in cases if c["name"] == "long_end_scene")
    assert len(ended["planned"]) == 3 and [s["finished"] for s in ended["planned"]] == [True, False, True]


def test_load_and_split_reads_the_written_csv(tmp_path):
    path = sd.write_scene_csv(str(tmp_path / "m-Scenes.csv"), [(0, 16), (16, 3200)], 24.0)
    scenes = m23.load_and_split_scenes(path, ",", 1500)
    assert [(s["Scene Number"], s["Start Frame"], s["End Frame"]) for s in scenes] == [("1", "1", "16"), ("2", "17", "1516"), ("3", "1517", "3016"), ("4", "3017", "3200")]


def _planned(engine="", tmp="out", **extra):
    row = dict(sd.scene_rows([(0, 12)], 24.0)[0], **extra)
    if engine:
        row["Engine"] = engine
    return m23.plan_scene_files(m23.split_scenes([row]), tmp, -1, exists=lambda p: False)[0]


def _args(*argv):
    return m23.build_parser().parse_args(["--color_video", "movie.mkv"] + list(argv))


def test_plan_commands_per_engine():
    v = os.path.join("out", "scene_1.mkv")
    d, mk = v + "_depth.mkv", v + "_mask.mkv"
    sbs = d + "_stereo.mkv"
    cmds = m23.plan_commands(_planned(), _args())
    assert [(c.step, c.tool) for c in cmds] == [(2, "video_da3"), (3, "generate_video_mask"), (4, "find_convergence_depth"), (5, "stereo_rerender"),
                                               (6, "stereo_crafter_infill")]
    assert cmds[0].argv == ["--color_video", v] and cmds[0].skip_if_exists == d
    assert cmds[1].argv == ["--color_video", v] and cmds[1].skip_if_exists == mk
    assert cmds[2].argv == ["--depth_video", d, "--mask_video", mk] and cmds[2].skip_if_exists == d + "_convergence_depths.json"
    assert cmds[3].argv == ["--color_video", v, "--convergence_file", d + "_convergence_depths.json", "--xfov_file", d + "_xfovs.json",
                            "--depth_video", d, "--infill_mask"] and cmds[3].skip_if_exists == sbs
    assert cmds[4].argv == ["--sbs_color_video", sbs, "--sbs_mask_video", sbs + "_infillmask.mkv"] and cmds[4].skip_if_exists == sbs + "_infilled.mkv"
    # the pass-through flags
    a = _args("--video_decoder", "device", "--video_encoder", "device", "--depth_generator", "p:d", "--mask_generator", "p:m", "--infill_generator", "p:i")
    cmds = m23.plan_commands(_planned(), a)
    codec = ["--video_decoder", "device", "--video_encoder", "device"]
    assert cmds[0].argv == ["--color_video", v, "--generator", "p:d"] + codec
    assert cmds[1].argv == ["--color_video", v, "--generator", "p:m"] + codec
    assert cmds[2].argv[-2:] == ["--video_decoder", "device"] and "--video_encoder" not in cmds[2].argv
    assert cmds[3].argv[-4:] == codec and cmds[4].argv[-6:] == ["--generator", "p:i"] + codec
    # vda: 42 degrees, the metric conversion of the dumps
    cmds = m23.plan_commands(_planned("vda"), _args("--infill_engine", "none"))
    assert [(c.step, c.tool) for c in cmds] == [(2, "video_metric_convert"), (3, "generate_video_mask"), (4, "find_convergence_depth"), (5, "stereo_rerender")]
    assert cmds[0].argv == ["--color_video", v, "--relative_depth", v + "_relative_depth.npy", "--metric_depth", v + "_metric_depth.npy", "--engine", "vda"]
    assert cmds[3].argv[cmds[3].argv.index("--xfov") + 1] == "42.0" and "--xfov_file" not in cmds[3].argv
    # depthcrafter / geometrycrafter: the single-frame reference twice, then the conversion; the x-fov is the mean of the first pass
    for engine in ("depthcrafter", "geometrycrafter"):
        cmds = m23.plan_commands(_planned(engine), _args("--infill_engine", "normals"))
        assert [(c.step, c.tool) for c in cmds] == [(2, "depth_engine_video"), (2, "depth_engine_video"), (2, "video_metric_convert"), (3, "generate_video_mask"),
                                                   (4, "find_convergence_depth"), (5, "stereo_rerender"), (6, "basic_nomal_infill")]
        org, single = d + "_org_xfovs.json", v + "_single_frame_depth.mkv"
        assert cmds[0].argv == ["--engine", "unik3d", "--color_video", v] and cmds[0].move == (d + "_xfovs.json", org) and cmds[0].skip_if_exists == org
        assert cmds[1].argv == ["--engine", "unik3d", "--xfov", m23.XFOV_TOKEN, "--color_video", v] and cmds[1].move == (d, single)
        assert cmds[1].xfov_from == org and cmds[1].skip_if_exists == single
        assert cmds[2].argv == ["--color_video", v, "--relative_depth", v + "_relative_depth.npy", "--depth_video", single, "--engine", "depthcrafter"]
        assert cmds[5].xfov_from == org and m23.XFOV_TOKEN in cmds[5].argv
    for engine in ("unik3d", "moge", "depthpro"):
        cmds = m23.plan_commands(_planned(engine), _args("--no_render"))
        assert [(c.step, c.tool) for c in cmds] == [(2, "depth_engine_video"), (3, "generate_video_mask"), (4, "find_convergence_depth")]
        assert cmds[0].argv == ["--engine", engine, "--color_video", v]
    # the infill engines
    for engine, tool in (("normals", "basic_nomal_infill"), ("stereocrafter", "stereo_crafter_infill"), ("m2svid", "m2svid_infill"),
                         ("stereo_dissoclusion_net", "stereo_dissoclusion_net_infill")):
        cmds = m23.plan_commands(_planned(), _args("--infill_engine", engine))
        assert cmds[-1].tool == tool and cmds[-1].step == 6
        assert ("--create_sbs_depth_video" in cmds[3].argv) == (engine == "stereo_dissoclusion_net")
    assert m23.plan_commands(_planned(), _args("--infill_engine", "m2svid"))[-1].argv[:2] == ["--color_video", v]
    assert m23.plan_commands(_planned(), _args("--infill_engine", "stereo_dissoclusion_net"))[-1].argv[4:6] == ["--sbs_depth_video", sbs + "_depth.mkv"]
    # the columns
    cmds = m23.plan_commands(_planned(Infill="No", Convergence="No"), _args())
    assert [c.step for c in cmds] == [2, 3, 4, 5] and "--infill_mask" not in cmds[3].argv and "--convergence_file" not in cmds[3].argv
    assert m23.file_to_concat(_planned(Infill="No"), _args()) == sbs and m23.file_to_concat(_planned(), _args()) == sbs + "_infilled.mkv"
    assert m23.file_to_concat(_planned(), _args("--infill_engine", "none")) == sbs
    # a finished scene takes none of steps 2-5
    done = _planned()
    done["finished"] = True
    assert [c.step for c in m23.plan_commands(done, _args())] == [6]
    with pytest.raises(ValueError, match="Engine"):
        m23.plan_commands(_planned("midas"), _args())
    with pytest.raises(NotImplementedError, match="masked phase correlation"):
        m23.plan_commands(_planned(), _args("--infill_engine", "inspatio_world"))
    assert m23.result_path(_args("--output_dir", "o")) == os.path.join("o", "movie.mkv_SBS.mkv") and "ffmpeg" in m23.mux_line(_args())


@pytest.fixture()
def driver():
    spec = importlib.util.spec_from_file_location("movie_2_3D_tool", os.path.join(REPO, "tools", "movie_2_3D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_resume_skips_what_exists(driver, tmp_path, monkeypatch):
    """Steps 2-6 over a directory of empty files: scene 1 has everything, scene 2 lacks its render and what follows."""
    out = str(tmp_path)
    rows = sd.scene_rows([(0, 12), (12, 24)], 24.0)
    ran = []

    def fake(name):
        def main(argv):
            ran.append(name)
            plan = [c for s in scenes for c in m23.plan_commands(s, args) if c.tool == name and list(c.argv) == list(argv)]
            open(plan[0].skip_if_exists, "w").close()
            return 0
        return main
    monkeypatch.setattr(driver, "tool_main", fake)
    args = _args("--output_dir", out, "--infill_engine", "normals")
    base = [os.path.join(out, f"scene_{k}.mkv") for k in (1, 2)]
    for b in base:
        for suffix in ("", "_depth.mkv", "_mask.mkv", "_depth.mkv_xfovs.json", "_depth.mkv_convergence_depths.json"):
            open(b + suffix, "w").close()
    for suffix in ("_depth.mkv_stereo.mkv", "_depth.mkv_stereo.mkv_infillmask.mkv", "_depth.mkv_stereo.mkv_infilled.mkv"):
        open(base[0] + suffix, "w").close()
    scenes = m23.plan_scene_files(m23.split_scenes(rows), out, -1)
    assert [s["finished"] for s in scenes] == [True, False]
    log = []
    driver.run_commands(args, scenes, log)
    assert log == [(5, "2", "stereo_rerender"), (6, "2", "basic_nomal_infill")] and ran == ["stereo_rerender", "basic_nomal_infill"]
    # the reference's rule (m23d:270): a scene whose _infilled file exists is finished, with or without its _stereo file
    os.remove(base[1] + "_depth.mkv_stereo.mkv")
    scenes = m23.plan_scene_files(m23.split_scenes(rows), out, -1)
    log = []
    driver.run_commands(args, scenes, log)
    assert [s["finished"] for s in scenes] == [True, True] and log == []


def test_the_driver_refuses_before_anything_is_written(driver, tmp_path):
    out = str(tmp_path / "out")
    movie = str(tmp_path / "movie.mkv")
    open(movie, "w").close()
    csv_path = sd.write_scene_csv(str(tmp_path / "s.csv"), [(0, 12)], 24.0)
    for argv, error, text in ((["--gui"], NotImplementedError, "gui"),
                              (["--infill_engine", "inspatio_world"], NotImplementedError, "masked phase correlation"),
                              (["--infill_engine", "magic"], ValueError, "unknown infill engine"),
                              (["--max_scene_frames", "0"], ValueError, "max_scene_frames"),
                              (["--scene_file", str(tmp_path / "none.csv")], FileNotFoundError, "scene file")):
        with pytest.raises(error, match=text):
            driver.run(m23.build_parser().parse_args(["--color_video", movie, "--output_dir", out] + argv))
    with pytest.raises(FileNotFoundError, match="color_video"):
        driver.run(m23.build_parser().parse_args(["--color_video", str(tmp_path / "none.mkv"), "--output_dir", out]))
    with pytest.raises(ValueError, match="need --color_video"):
        driver.run(m23.build_parser().parse_args(["--output_dir", out]))
    assert not os.path.exists(out) and sorted(os.listdir(tmp_path)) == ["movie.mkv", "s.csv"]
    # an unknown Engine column: the output directory is made, no scene clip is
    with open(csv_path) as fh:
        lines = fh.read().splitlines()
    with open(csv_path, "w") as fh:
        fh.write("\n".join([lines[0], lines[1] + ",Engine", lines[2] + ",midas"]) + "\n")
    with pytest.raises(ValueError, match="Engine"):
        driver.run(m23.build_parser().parse_args(["--color_video", movie, "--output_dir", out, "--scene_file", csv_path]))
    assert os.listdir(out) == []
