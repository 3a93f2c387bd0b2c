"""Near-plane clipping without a GPU: the exported symbol, the renderer's keyword check, the command line's flag and its refusals."""
import ctypes as C

import pytest


def test_symbol_is_exported_and_config_record_keeps_its_size():
    from metric_depth_video_toolbox_amd import _lib
    assert "mdvt_set_near_clip" in _lib.SYMBOLS
    assert "mdvt_set_near_clip" in _lib.exported_symbols()
    assert C.sizeof(_lib.MdvtConfig) == 48


@pytest.mark.parametrize("value", [2, -1, 0.5, "yes", None, 1.0])
def test_renderer_keyword_is_checked_before_any_device_call(value):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    with pytest.raises(ValueError, match="near_clip"):
        sr.StereoRerenderer(64, 48, near_clip=value)
    for ok in (True, False, 0, 1):
        sr.check_near_clip(ok)


def _parse(*flags):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    return sr.build_arg_parser().parse_args(["--depth_video", "d.npy", "--xfov", "50", *flags])


def test_cli_flag_maps_to_the_renderer_keyword(monkeypatch, tmp_path):
    from metric_depth_video_toolbox_amd import clip
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    assert _parse().near_clip is False and _parse("--near_clip").near_clip is True
    for flags in (("--near_clip",), ("--near_clip", "--infill_mask", "--dont_place_points_in_edges", "--green_and_black_infill_mask"),
                  ("--near_clip", "--remove_edges", "--dont_place_points_in_edges"), ("--near_clip", "--infill_mask", "--dont_remove_edges"),
                  ("--near_clip", "--multisample", "4"), ("--near_clip", "--render_as_pointcloud", "--infill_mask"),
                  ("--near_clip", "--render_as_pointcloud", "--create_sbs_depth_video")):
        assert sr.near_clip_conflict(_parse(*flags)) is None, flags
    seen = {}

    def fake_run(depth_path, color_path, **kw):
        seen.update(kw)
        import numpy as np
        return np.ones((1, 2)), "out"
    monkeypatch.setattr(clip, "run", fake_run)
    dp = tmp_path / "d.npy"
    dp.write_bytes(b"x")
    assert sr.main(["--depth_video", str(dp), "--xfov", "50", "--near_clip"]) == 0
    assert seen["near_clip"] is True
    assert sr.main(["--depth_video", str(dp), "--xfov", "50"]) == 0
    assert seen["near_clip"] is False


def test_renderer_for_passes_the_keyword(monkeypatch):
    from metric_depth_video_toolbox_amd import clip
    got = {}

    class Fake:
        def __init__(self, *a, **kw):
            got.update(kw)
    monkeypatch.setattr(clip, "StereoRerenderer", Fake)

    class Clip:
        mode_flags, ipd_m, W, H, max_depth, master_xfov = 0, 0.065, 64, 48, 100, 45.0
    clip.renderer_for(Clip(), 0, None, True)
    assert got.get("near_clip") is True
    got.clear()
    clip.renderer_for(Clip(), 0)
    assert "near_clip" not in got


@pytest.mark.parametrize("flags,word", [(("--infill_mask",), "--dont_place_points_in_edges"),
                                        (("--remove_edges",), "--dont_place_points_in_edges"),
                                        (("--infill_mask", "--dont_place_points_in_edges"), "--green_and_black_infill_mask"),
                                        (("--do_basic_infill", "--dont_place_points_in_edges"), "--do_basic_infill"),
                                        (("--touchly0",), "--touchly0"), (("--touchly1",), "--touchly1"),
                                        (("--create_sbs_depth_video",), "--create_sbs_depth_video"),
                                        (("--normal_infill", "--infill_mask", "--dont_place_points_in_edges",
                                          "--green_and_black_infill_mask"), "--normal_infill")])
def test_cli_refuses_what_clipping_cannot_serve_before_reading_frames(tmp_path, flags, word):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    assert word in sr.near_clip_conflict(_parse("--near_clip", *flags))
    assert sr.near_clip_conflict(_parse(*flags)) is None
    dp = tmp_path / "d.npy"
    dp.write_bytes(b"not a frame dump")          # never read: the refusal comes first
    with pytest.raises(ValueError, match=word):
        sr.main(["--depth_video", str(dp), "--xfov", "50", "--near_clip", *flags])
