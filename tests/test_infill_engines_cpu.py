"""The two further infill engines' host side -- no GPU: the binding of the two entry points of include/mdvt_infill_engines.h, the
composed finish of tests/infill_engines_ref.py pinned against the C oracle's normal_infill (which tests/golden/normal_infill.npz holds
to the reference's own function), and the two command lines."""
import hashlib
import os
import re

import numpy as np
import pytest

import infill_engines_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mdvt_m2svid_prepare_eye", "mdvt_model_infill_finish"]


def test_the_entry_points_are_exported_outside_the_main_header():
    import ctypes
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "mdvt_infill_engines.h")).read()
    body = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", body)))
    assert declared == sorted(_lib.INFILL_ENGINE_SYMBOLS) == NAMES
    others = (_lib.SYMBOLS + _lib.DECODE_SYMBOLS + _lib.STREAM_DECODE_SYMBOLS + _lib.CONVERGENCE_SYMBOLS + _lib.METRIC_ALIGN_SYMBOLS +
              _lib.INFILL_ADAPTER_SYMBOLS)
    main = open(os.path.join(REPO, "include", "mdvt.h"), "rb").read()
    adapter = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "mdvt_infill_adapter.h")).read(), flags=re.S)
    tuning = ctypes.CDLL(_lib.lib_path("tuning"))
    for s in NAMES:
        assert hasattr(L, s) and hasattr(tuning, s) and s not in others and s.encode() not in main and s not in adapter
    # include/mdvt.h is byte for byte what ABI 0.15 shipped; the adapter's header keeps exactly its four declarations
    assert hashlib.sha256(main).hexdigest() == "5f1d16f6a06b01ef262e293213d5ed895e2c27a0172feeb538a2b486b3720e04"
    assert L.mdvt_version() == 15
    assert sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", adapter))) == sorted(_lib.INFILL_ADAPTER_SYMBOLS)
    for doc in ("RESTATED, not observed", "Footprint: the first 3 * image_w bytes", "Footprint: the first 3 * width bytes", "No workspace",
                "Workspace: a scratch block of the context", "bytes per pixel", "No byte parity with cv2"):
        assert doc in hdr, doc
    # the argument counts of the binding are the header's
    for s in NAMES:
        args = re.search(s + r"\s*\((.*?)\)\s*;", body, flags=re.S).group(1)
        assert len(getattr(L, s).argtypes) == args.count(",") + 1, s


# ---- the composed finish against the oracle's normal_infill ---------------------------------------------------------------------

def _cases(golden):
    z = golden("normal_infill")
    for tag in ("n1", "n2"):
        yield tag, z[tag + "_img"], z[tag + "_mask"]
    rng = np.random.default_rng(77)
    for k, (W, H) in enumerate(((37, 23), (64, 48), (130, 33))):
        for kind in ("mixed", "borders", "pixels", "directions", "deep", "zero_channel", "all"):
            yield f"{W}x{H} {kind}", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), E.finish_masks(rng, H, W, kind)


def test_the_composed_finish_is_the_tail_of_normal_infill(orc, golden):
    """With normal_infill's own filled image standing in as the model, the composition equals orc_normal_infill bit for bit: the box
    mean is only read at bg pixels and the work image only blackened there, so `img as it is` changes nothing."""
    ran = 0
    for tag, img, mask in _cases(golden):
        want, st = orc.normal_infill(img, mask, want_stages=True)
        got, mine = E.finish_stages(img, st["filled"], mask, orc)
        assert np.array_equal(mine["bg"], st["bg"]) and np.array_equal(mine["grown"], st["grown"]), tag
        assert np.array_equal(mine["work"], st["merged"]), tag
        assert np.array_equal(got, want), tag
        ran += 1
    assert ran == 23
    z = golden("normal_infill")                                    # ... and normal_infill is the reference's own function there
    for tag in ("n1", "n2"):
        assert np.array_equal(orc.normal_infill(z[tag + "_img"], z[tag + "_mask"]), z[tag + "_out"])


def test_the_finish_test_inputs_are_what_they_claim(orc):
    rng = np.random.default_rng(3)
    H, W = 40, 70
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    model = 255 - img
    out, st = E.finish_stages(img, model, E.finish_masks(rng, H, W, "none"), orc)
    assert np.array_equal(out, img) and not st["bg"].any() and not st["grown"].any()
    _, st = E.finish_stages(img, model, E.finish_masks(rng, H, W, "all"), orc)
    assert st["bg"].all()
    m = E.finish_masks(rng, H, W, "zero_channel")
    _, st = E.finish_stages(img, model, m, orc)
    marching = (m != 0).any(axis=-1)
    assert marching.sum() > st["bg"].sum() > 0 and st["marks"].any()       # some pixels march without being bg
    m = E.finish_masks(rng, H, W, "deep")
    _, st = E.finish_stages(img, model, m, orc)
    assert W - 2 > 2 * 30 and st["bg"].sum() == (H - 2) * (W - 2) and st["marks"].any() and not st["grown"].all()
    m = E.finish_masks(rng, H, W, "directions")
    _, st = E.finish_stages(img, model, m, orc)
    dirs = {(int(np.sign(int(r) - 127.5 if abs(int(r) - 127.5) > 1 else 0)), int(np.sign(int(g) - 127.5 if abs(int(g) - 127.5) > 1 else 0)))
            for r, g in m[m.any(axis=-1)][:, :2]}
    assert len(dirs) == 8 and st["marks"].sum() >= 8                     # four quadrants and four axis directions, each marking a lower side
    _, st = E.finish_stages(img, model, E.finish_masks(rng, H, W, "borders"), orc)
    g = st["grown"]
    assert st["bg"][0, 0] and st["bg"][H - 1, W - 1] and g[0].any() and g[-1].any() and g[:, 0].any() and g[:, -1].any()       # the blur reaches every border


def test_m2s_restatement_on_a_clip_without_holes(orc):
    """The schedule's calls are the StereoCrafter step's, and a clip without holes comes back as it went in, blended or not."""
    import infill_adapter_ref as R
    n = 31
    rng = np.random.default_rng(n)
    color = rng.integers(0, 256, (n, 8, 16, 3), dtype=np.uint8)
    org = rng.integers(0, 256, (n, 6, 10, 3), dtype=np.uint8)
    for blend in (False, True):
        out, calls = E.m2s_run_clip(color, np.zeros((0, 8, 16, 3), np.uint8), org, 24.0, None, orc, blend, (8, 8), (4, 4))
        assert calls == R.run_clip(color, np.zeros((0, 8, 16, 3), np.uint8), 24.0, None, orc, model_size=(8, 8))[1] == [(True, False, 25), (False, True, 12)]
        assert np.array_equal(out, color)
    im, og, mk, cnt = E.m2s_prepare_eye(color[:2], np.zeros_like(color[:2]), org[:2], 0, (8, 8), (4, 4))
    assert im.shape == og.shape == (2, 8, 8, 3) and mk.shape == (2, 4, 4) and not cnt.any()
    assert np.array_equal(im[0], color[0, :, 7::-1])               # equal sizes: the mirrored copy


# ---- the command lines ----------------------------------------------------------------------------------------------------------

def test_m2svid_cli_parses_the_reference_flags_and_its_own():
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    base = ["--color_video", "o.mkv", "--sbs_color_video", "a.mkv", "--sbs_mask_video", "b.mkv"]
    a = m2s.build_parser().parse_args(base)
    assert (a.max_frames, a.num_inference_steps, a.apply_edge_blending, a.generator, a.batch, a.video_decoder, a.video_encoder) == \
        (-1, 5, False, "m2svid", 8, "host", "host")
    a = m2s.build_parser().parse_args(base + ["--max_frames", "7", "--num_inference_steps", "3", "--apply_edge_blending", "--generator", "pkg.mod:fn",
                                              "--batch", "4", "--video_decoder", "device_all", "--video_encoder", "device"])
    assert (a.max_frames, a.num_inference_steps, a.apply_edge_blending, a.generator, a.batch, a.video_decoder, a.video_encoder) == \
        (7, 3, True, "pkg.mod:fn", 4, "device_all", "device")
    with pytest.raises(SystemExit):
        m2s.build_parser().parse_args(base[2:])                    # --color_video is required
    with pytest.raises(SystemExit):
        m2s.build_parser().parse_args(base + ["--video_encoder", "gpu"])
    assert (m2s.IMAGE_W, m2s.IMAGE_H, m2s.MASK_W, m2s.MASK_H) == (512, 512, 64, 64)
    assert "generate(frames, masks, org_frames, fps) -> frames" in m2s.__doc__ and "UNTESTED" in m2s.M2SVidGenerator.__doc__


def test_sdn_cli_parses_the_reference_flags_and_its_own():
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    base = ["--sbs_color_video", "a.mkv", "--sbs_mask_video", "b.mkv", "--sbs_depth_video", "d.mkv"]
    a = sdn.build_parser().parse_args(base)
    assert (a.max_frames, a.generator, a.batch, a.video_decoder, a.video_encoder) == (-1, "stereo_dissoclusion_net", 8, "host", "host")
    a = sdn.build_parser().parse_args(base + ["--max_frames", "2", "--generator", "pkg.mod:fn", "--batch", "3", "--video_decoder", "device",
                                              "--video_encoder", "device"])
    assert (a.max_frames, a.generator, a.batch, a.video_decoder, a.video_encoder) == (2, "pkg.mod:fn", 3, "device", "device")
    with pytest.raises(SystemExit):
        sdn.build_parser().parse_args(base[:4])                    # --sbs_depth_video is required
    assert "generate(image, infill_mask, depth) -> image" in sdn.__doc__ and "UNTESTED" in sdn.StereoDissoclusionNetGenerator.__doc__


def _lists(tmp_path, counts):
    paths = []
    for k, n in enumerate(counts):
        p = tmp_path / f"list{k}.txt"
        p.write_text("# a comment\n\n" + "".join(f"missing_{k}_{i}.mkv\n" for i in range(n)))
        paths.append(str(p))
    return paths


def test_mismatched_list_lengths_are_refused_before_any_file_is_read(tmp_path):
    """The entries name files that do not exist: a length mismatch is reported before anything is opened (and before the generator
    is loaded)."""
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    for counts in ((2, 2, 3), (2, 1, 2), (3, 2, 2)):
        c, m, o = _lists(tmp_path, counts)
        with pytest.raises(ValueError, match="List length mismatch"):
            m2s.main(["--sbs_color_video", c, "--sbs_mask_video", m, "--color_video", o, "--generator", "no.such.module:fn"])
        with pytest.raises(ValueError, match="List length mismatch"):
            sdn.main(["--sbs_color_video", c, "--sbs_mask_video", m, "--sbs_depth_video", o, "--generator", "no.such.module:fn"])
    c, m, o = _lists(tmp_path, (2, 2, 2))
    assert m2s.triples_from_arguments(o, c, m) == [(f"missing_0_{i}.mkv", f"missing_1_{i}.mkv", f"missing_2_{i}.mkv") for i in range(2)]
    assert sdn.triples_from_arguments(c, m, o) == m2s.triples_from_arguments(o, c, m)
    with pytest.raises(ValueError, match="must also be"):
        m2s.main(["--sbs_color_video", c, "--sbs_mask_video", "b.mkv", "--color_video", o])
    with pytest.raises(ValueError, match="must also be"):
        sdn.main(["--sbs_color_video", c, "--sbs_mask_video", m, "--sbs_depth_video", "d.mkv"])
    assert not [f for f in os.listdir(tmp_path) if "infilled" in f]


def test_cli_refusals_leave_no_file_behind(tmp_path):
    from metric_depth_video_toolbox_amd import m2svid_infill as m2s
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn
    files = {}
    for name, shape in (("x", (2, 8, 16, 3)), ("x_mask", (2, 8, 16, 3)), ("org", (2, 6, 10, 3)), ("x_depth", (2, 8, 16, 3))):
        files[name] = str(tmp_path / (name + ".npy"))
        np.save(files[name], np.zeros(shape, dtype=np.uint8))
    before = sorted(os.listdir(tmp_path))
    m_base = ["--sbs_color_video", files["x"], "--sbs_mask_video", files["x_mask"], "--color_video", files["org"]]
    s_base = ["--sbs_color_video", files["x"], "--sbs_mask_video", files["x_mask"], "--sbs_depth_video", files["x_depth"]]
    with pytest.raises(SystemExit) as e:                           # the default models are not installed: one clear line each
        m2s.main(m_base)
    assert "m2svid generator needs" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        sdn.main(s_base)
    assert "stereo_dissoclusion_net generator needs" in str(e.value) and "\n" not in str(e.value)
    for mod, base in ((m2s, m_base), (sdn, s_base)):
        for extra, text in ((["--generator", "nocolon"], "pkg.module:callable"), (["--generator", "os.path:nothing_here"], "no callable"),
                            (["--generator", "os.path:join", "--max_frames", "0"], "max_frames")):
            with pytest.raises(SystemExit) as e:
                mod.main(base + extra)
            assert text in str(e.value)
        with pytest.raises(SystemExit) as e:
            mod.main(["--sbs_color_video", str(tmp_path / "missing.mkv")] + base[2:] + ["--generator", "os.path:join"])
        assert "does not exist" in str(e.value)
    assert sorted(os.listdir(tmp_path)) == before
    assert m2s.load_generator("os.path:join") is os.path.join and sdn.load_generator("os.path:join") is os.path.join
