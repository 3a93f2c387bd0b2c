"""CPU-only tests of the opt-in heap order of the infill-mask completion: the library exports both entry points, the Python
bindings list them, the CLI carries --inpaint_order (default: the level order) and the ABI version is unchanged."""
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAP_SYMBOLS = ("mdvt_finish_infill_mask_heap", "mdvt_finish_infill_mask_heap_stereo")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from metric_depth_video_toolbox_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def test_library_exports_the_heap_entry_points(lib):
    exported = lib.exported_symbols()
    for sym in HEAP_SYMBOLS:
        assert sym in lib.SYMBOLS
        assert sym in exported
    L = lib.load()
    assert len(L.mdvt_finish_infill_mask_heap.argtypes) == 10
    assert len(L.mdvt_finish_infill_mask_heap_stereo.argtypes) == 12


def test_header_declares_them_and_the_version_stays(lib):
    hdr = open(os.path.join(REPO, "include", "mdvt.h")).read()
    for sym in HEAP_SYMBOLS:
        assert sym + "(" in hdr
    assert lib.load().mdvt_version() == (0 << 16) | 15


def test_cli_flag_defaults_to_the_level_order():
    from metric_depth_video_toolbox_amd.stereo_rerender import INPAINT_ORDERS, build_arg_parser
    base = ["--depth_video", "d.npy", "--xfov", "45"]
    ap = build_arg_parser()
    assert INPAINT_ORDERS == ("levels", "heap")
    assert ap.parse_args(base).inpaint_order == "levels"
    assert ap.parse_args(base + ["--infill_mask", "--inpaint_order", "heap"]).inpaint_order == "heap"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--inpaint_order", "fifo"])
    help_text = ap.format_help()
    assert "--inpaint_order" in help_text and "not a reference flag" in " ".join(help_text.split())


def test_clip_run_takes_the_order():
    import inspect
    from metric_depth_video_toolbox_amd import clip
    assert inspect.signature(clip.run).parameters["inpaint_order"].default == "levels"
    assert inspect.signature(clip.render_clip).parameters["inpaint_order"].default == "levels"
