"""infill_clip's pure parts, which the four infill scripts share: the list-file arguments, the common command-line flags, the
arithmetic of the black-padded mask fetch and the chunk schedule.  No GPU."""
import argparse

import pytest

from metric_depth_video_toolbox_amd import infill_clip as ic


def _lists(tmp_path, counts, suffix=".txt"):
    paths = []
    for k, n in enumerate(counts):
        p = tmp_path / f"list{k}{suffix}"
        p.write_text("# a comment\n\n" + "".join(f"  clip_{k}_{i}.mkv \n#skipped\n\n" for i in range(n)))
        paths.append(str(p))
    return paths


def test_tuples_from_arguments_single_clips_and_lists(tmp_path):
    assert ic.tuples_from_arguments([("a", "x.mkv"), ("b", "y.mkv")]) == [("x.mkv", "y.mkv")]
    assert ic.tuples_from_arguments([("a", "x.npy"), ("b", "y.txt"), ("c", "z.npy")]) == [("x.npy", "y.txt", "z.npy")]      # only the leading one decides
    for suffix in (".txt", ".TXT"):
        a, b, c = _lists(tmp_path, (2, 2, 2), suffix)
        assert ic.is_txt(a) and not ic.is_txt("x.mkv") and not ic.is_txt(None)
        assert ic.read_list_file(a) == ["clip_0_0.mkv", "clip_0_1.mkv"]          # comment and blank lines skipped, entries stripped
        assert ic.tuples_from_arguments([("a", a), ("b", b)]) == [(f"clip_0_{i}.mkv", f"clip_1_{i}.mkv") for i in range(2)]
        assert ic.tuples_from_arguments([("a", a), ("b", b), ("c", c)]) == [(f"clip_0_{i}.mkv", f"clip_1_{i}.mkv", f"clip_2_{i}.mkv") for i in range(2)]


def test_tuples_from_arguments_error_messages_are_the_scripts(tmp_path):
    a, b, c = _lists(tmp_path, (2, 1, 3))
    with pytest.raises(ValueError) as e:
        ic.tuples_from_arguments([("sbs_color_video", a), ("sbs_mask_video", "y.npy")])
    assert str(e.value) == "If --sbs_color_video is a .txt file, then --sbs_mask_video must also be a .txt file."
    for values in ((b, "z.mkv"), ("y.mkv", c), ("y.mkv", "z.mkv")):
        with pytest.raises(ValueError) as e:
            ic.tuples_from_arguments([("sbs_color_video", a), ("sbs_mask_video", values[0]), ("color_video", values[1])])
        assert str(e.value) == "If --sbs_color_video is a .txt file, then --sbs_mask_video and --color_video must also be .txt files."
    with pytest.raises(ValueError) as e:
        ic.tuples_from_arguments([("sbs_color_video", a), ("sbs_mask_video", b)])
    assert str(e.value) == f"List length mismatch: {a} has 2 entries, {b} has 1 entries."
    for second, third, n2, n3 in ((b, c, 1, 3), (a, c, 2, 3), (b, a, 1, 2)):
        with pytest.raises(ValueError) as e:
            ic.tuples_from_arguments([("sbs_color_video", a), ("sbs_mask_video", second), ("sbs_depth_video", third)])
        assert str(e.value) == f"List length mismatch: {a} has 2 entries, {second} has {n2} entries, {third} has {n3} entries."


def test_the_scripts_wrappers_keep_their_argument_and_tuple_order(tmp_path):
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, m2svid_infill as m2s, stereo_dissoclusion_net_infill as sdn
    a, b, c = _lists(tmp_path, (2, 2, 2))
    want = [(f"clip_0_{i}.mkv", f"clip_1_{i}.mkv", f"clip_2_{i}.mkv") for i in range(2)]
    assert bni.pairs_from_arguments(a, b) == [w[:2] for w in want] and bni.pairs_from_arguments("x", "y") == [("x", "y")]
    assert sdn.triples_from_arguments(a, b, c) == want and sdn.triples_from_arguments("x", "y", "z") == [("x", "y", "z")]
    assert m2s.triples_from_arguments(c, a, b) == want and m2s.triples_from_arguments("o", "x", "y") == [("x", "y", "o")]
    with pytest.raises(ValueError) as e:
        m2s.triples_from_arguments("o.mkv", a, b)
    assert str(e.value) == "If --sbs_color_video is a .txt file, then --sbs_mask_video and --color_video must also be .txt files."
    with pytest.raises(ValueError) as e:
        sdn.triples_from_arguments(a, b, "d.mkv")
    assert str(e.value) == "If --sbs_color_video is a .txt file, then --sbs_mask_video and --sbs_depth_video must also be .txt files."


def test_common_flags_are_the_same_in_all_four_parsers():
    from metric_depth_video_toolbox_amd import basic_nomal_infill as bni, m2svid_infill as m2s, stereo_crafter_infill as sci
    from metric_depth_video_toolbox_amd import stereo_dissoclusion_net_infill as sdn

    def flags(parser):
        return {a.option_strings[0]: a for a in parser._actions if a.option_strings and a.option_strings[0] != "-h"}
    common = flags(ic.add_common_flags(argparse.ArgumentParser()))
    assert {k: (a.default, a.choices, a.type, a.required) for k, a in common.items()} == {
        "--max_frames": (-1, None, int, False), "--batch": (8, None, int, False),
        "--video_decoder": ("host", ("host", "device", "device_all"), None, False), "--video_encoder": ("host", ("host", "device"), None, False)}
    for mod in (bni, sci, m2s, sdn):
        theirs = flags(mod.build_parser())
        for name, a in common.items():
            b = theirs[name]
            assert (b.default, b.choices, b.type, b.required, b.dest, b.help) == (a.default, a.choices, a.type, a.required, a.dest, a.help), (mod.__name__, name)
        assert theirs["--sbs_color_video"].required and theirs["--sbs_mask_video"].required


@pytest.mark.parametrize("a,b,mask_len,want", [
    (0, 8, 20, (8, 0)), (8, 16, 20, (8, 0)),          # the mask clip is longer than the clip
    (8, 16, 16, (8, 0)),                              # as long as the clip: the last batch
    (8, 16, 11, (3, 5)), (8, 16, 15, (7, 1)),         # ends inside the batch
    (8, 16, 8, (0, 8)), (8, 16, 3, (0, 8)),           # ended before the batch
    (0, 8, 0, (0, 8)), (24, 25, 0, (0, 1)),           # no mask frames at all
    (5, 6, 6, (1, 0)), (5, 6, 5, (0, 1)),             # one frame
])
def test_mask_split(a, b, mask_len, want):
    have, blank = ic.mask_split(a, b, mask_len)
    assert (have, blank) == want and have + blank == b - a and have >= 0 and blank >= 0


def test_chunk_schedule_is_the_one_stereo_crafter_infill_exports():
    from metric_depth_video_toolbox_amd import stereo_crafter_infill as sci
    assert (sci.FRAMES_CHUNK, sci.OVERLAP) == (ic.FRAMES_CHUNK, ic.OVERLAP) == (25, 6)
    for n in range(1, 61):
        sched = ic.chunk_schedule(n)
        assert sched == sci.chunk_schedule(n)
        assert [t for *_, (a, b) in sched for t in range(a, b)] == list(range(n))
    with pytest.raises(ValueError):
        ic.chunk_schedule(0)
