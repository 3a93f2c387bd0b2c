"""The multisampling setting without a GPU: the ABI's config record, the renderer's keyword checks and the command line's flags."""
import ctypes as C

import pytest


def test_config_record_keeps_its_size_and_offsets():
    from metric_depth_video_toolbox_amd import _lib
    cfg = _lib.MdvtConfig
    assert C.sizeof(cfg) == 48
    assert cfg.subpixel_bits.offset == 40
    assert (cfg.samples.offset, cfg.sample_pattern.offset, cfg.sample_resolve.offset) == (44, 46, 47)   # the old reserved2
    assert (cfg.samples.size, cfg.sample_pattern.size, cfg.sample_resolve.size) == (2, 1, 1)
    c = cfg()
    assert (c.samples, c.sample_pattern, c.sample_resolve) == (0, 0, 0)      # all zero: single sample, as before


@pytest.mark.parametrize("kw,word", [(dict(samples=2), "samples"), (dict(samples=8), "samples"), (dict(samples=-1), "samples"),
                                     (dict(samples=True), "samples"), (dict(samples=4, sample_pattern=2), "sample_pattern"),
                                     (dict(samples=4, sample_resolve=2), "sample_resolve"),
                                     (dict(samples=4, sample_pattern=-1), "sample_pattern")])
def test_renderer_keywords_out_of_range_raise_before_any_device_call(kw, word):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    with pytest.raises(ValueError, match=word):
        sr.StereoRerenderer(64, 48, **kw)


def _parse(*flags):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    return sr.build_arg_parser().parse_args(["--depth_video", "d.npy", "--xfov", "50", *flags])


def test_cli_flags_map_to_the_renderer_keywords():
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    assert sr.multisample_kwargs(_parse()) == {}
    assert sr.multisample_kwargs(_parse("--multisample", "off", "--sample_pattern", "swiftshader")) == {}
    assert sr.multisample_kwargs(_parse("--multisample", "4")) == dict(samples=4, sample_pattern=0, sample_resolve=0)
    assert sr.multisample_kwargs(_parse("--multisample", "4", "--sample_pattern", "swiftshader")) == \
        dict(samples=4, sample_pattern=1, sample_resolve=1)
    for flags in ((), ("--multisample", "4"), ("--multisample", "4", "--infill_mask", "--dont_place_points_in_edges",
                                                  "--green_and_black_infill_mask"),
                  ("--multisample", "4", "--remove_edges", "--dont_place_points_in_edges"),
                  ("--multisample", "4", "--infill_mask", "--dont_remove_edges"), ("--multisample", "4", "--vr180")):
        assert sr.multisample_conflict(_parse(*flags)) is None, flags
    with pytest.raises(SystemExit):
        _parse("--multisample", "2")


@pytest.mark.parametrize("flags,word", [(("--infill_mask",), "--dont_place_points_in_edges"),
                                        (("--remove_edges",), "--dont_place_points_in_edges"),
                                        (("--infill_mask", "--dont_place_points_in_edges"), "--green_and_black_infill_mask"),
                                        (("--do_basic_infill", "--dont_place_points_in_edges"), "--do_basic_infill"),
                                        (("--touchly0",), "--touchly0"), (("--touchly1",), "--touchly1"),
                                        (("--create_sbs_depth_video",), "--create_sbs_depth_video")])
def test_cli_refuses_what_multisampling_cannot_serve_before_reading_frames(tmp_path, flags, word):
    from metric_depth_video_toolbox_amd import stereo_rerender as sr
    assert word in sr.multisample_conflict(_parse("--multisample", "4", *flags))
    assert sr.multisample_conflict(_parse(*flags)) is None
    dp = tmp_path / "d.npy"
    dp.write_bytes(b"not a frame dump")          # never read: the refusal comes first
    with pytest.raises(ValueError, match=word):
        sr.main(["--depth_video", str(dp), "--xfov", "50", "--multisample", "4", *flags])
