"""metric_depth_video_toolbox_amd/step_clip.py on the host: what the model-step tools' host modules export is the shared function or
gives what it gave before, the frame rule is the reference's counting loop, the session's host phase refuses in the tools' order with
their texts and reaches no GPU, the list loop keeps its order, and the module takes no tensor's address."""
import argparse
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_modules_names_are_the_shared_functions_or_give_what_they_gave(tmp_path):
    from metric_depth_video_toolbox_amd import depth_engines, infill_clip, step_clip, video_da3, video_mask, video_mvsa
    lst = tmp_path / "clips.txt"
    lst.write_text("# a list\n\n a.mkv \nb.mkv\n")
    for host in (video_da3, depth_engines, video_mask, video_mvsa):
        assert host.clips_from_argument is step_clip.clips_from_argument
        assert host.clips_from_argument(str(lst)) == ["a.mkv", "b.mkv"] and host.clips_from_argument("a.mkv") == ["a.mkv"]
    assert depth_engines.frames_to_write is step_clip.frames_to_write and video_mask.frames_to_write is step_clip.frames_to_write
    assert (step_clip.is_txt, step_clip.read_list_file, step_clip.callable_from_spec) == \
        (infill_clip.is_txt, infill_clip.read_list_file, infill_clip.callable_from_spec)
    # the file names, as the hosts' own CPU tests state them
    assert video_da3.output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_xfovs.json",
                                                "x.mkv_depth.mkv_transformations.json")
    assert video_da3.output_paths("x.npy", video=False)[:2] == ("x.npy_tmp_depth.npy", "x.npy_depth.npy")
    assert depth_engines.engine_output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_xfovs.json")
    assert depth_engines.engine_output_paths("x.npy", False) == ("x.npy_tmp_depth.npy", "x.npy_depth.npy", "x.npy_depth.npy_xfovs.json")
    assert depth_engines.promptda_output_paths("d.mkv") == ("d.mkv_tmp_upscaled.mkv", "d.mkv_upscaled.mkv")
    assert depth_engines.promptda_output_paths("d.npy", False) == ("d.npy_tmp_upscaled.npy", "d.npy_upscaled.npy")
    assert video_mask.output_paths("x.mkv") == ("x.mkv_tmp_mask.mkv", "x.mkv_mask.mkv")
    assert video_mask.output_paths("x.npy", video=False) == ("x.npy_tmp_mask.npy", "x.npy_mask.npy")
    assert video_mvsa.output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_cv_scales.json")
    assert video_mvsa.output_paths("x.npy", False) == ("x.npy_tmp_depth.npy", "x.npy_depth.npy", "x.npy_depth.npy_cv_scales.json")
    # the writers: the bytes json.dumps gives a list of Python floats
    values = [np.float32(0.1), np.float64(2.5), 3]
    want = json.dumps([float(v) for v in values]).encode()
    for write in (depth_engines.write_xfovs, video_mvsa.write_scales):
        write(str(tmp_path / "v.json"), values)
        assert (tmp_path / "v.json").read_bytes() == want
    T = [np.eye(4), np.arange(16.0).reshape(4, 4)]
    video_da3.write_json_files(str(tmp_path / "x.json"), str(tmp_path / "t.json"), values, T)
    assert (tmp_path / "x.json").read_bytes() == want
    assert (tmp_path / "t.json").read_bytes() == json.dumps([np.asarray(t, np.float64).tolist() for t in T]).encode()


def test_the_parsers_keep_their_flags_and_defaults():
    from metric_depth_video_toolbox_amd import depth_engines, video_da3, video_mask, video_mvsa
    from metric_depth_video_toolbox_amd.clip_io import VIDEO_DECODERS, VIDEO_ENCODERS
    parsers = ((video_da3.build_parser(), None), (depth_engines.build_engine_parser(), 8), (depth_engines.build_promptda_parser(), 4),
               (video_mask.build_parser(), None), (video_mvsa.build_parser(), 8))
    for p, batch in parsers:
        by_flag = {a.option_strings[0]: a for a in p._actions if a.option_strings}
        dec, enc = by_flag["--video_decoder"], by_flag["--video_encoder"]
        assert (dec.default, tuple(dec.choices), enc.default, tuple(enc.choices)) == ("host", tuple(VIDEO_DECODERS), "host", tuple(VIDEO_ENCODERS))
        assert ("--batch" in by_flag) == (batch is not None)
        if batch is not None:
            assert by_flag["--batch"].default == batch and by_flag["--batch"].type is int
            assert by_flag["--batch"].help.startswith("not a reference flag: frames per read")
    assert "per read-back" in {a.option_strings[0]: a for a in parsers[1][0]._actions if a.option_strings}["--batch"].help
    assert "per resize call" in {a.option_strings[0]: a for a in parsers[4][0]._actions if a.option_strings}["--batch"].help


def test_frames_to_write_is_the_references_counting_loop():
    from metric_depth_video_toolbox_amd import step_clip

    def reference_loop(n_in_file, max_frames):                       # u3d:155-163, gvm:85-109 as written
        frame_n, written = 0, 0
        for _ in range(n_in_file):
            frame_n += 1
            if max_frames != -1 and max_frames < frame_n:
                break
            written += 1
        return written
    for n in range(0, 6):
        for m in range(-1, 7):
            assert step_clip.frames_to_write(n, m) == reference_loop(n, m), (n, m)


def test_the_host_phase_refuses_in_order_writes_nothing_and_reaches_no_gpu(tmp_path, monkeypatch):
    import torch
    from metric_depth_video_toolbox_amd import _lib, step_clip

    def no_gpu(*a, **k):
        raise AssertionError("the host phase reached the GPU")
    monkeypatch.setattr(_lib, "Context", no_gpu)
    monkeypatch.setattr(torch.cuda, "current_device", no_gpu)
    frames, planes = str(tmp_path / "frames.npy"), str(tmp_path / "planes.npy")
    np.save(frames, np.zeros((3, 4, 5, 3), np.uint8))
    np.save(planes, np.zeros((3, 4, 5), np.uint8))
    before = sorted(os.listdir(tmp_path))
    missing = Exception("the tool's own words")

    def host_phase(path, decoder="host", encoder="host", max_frames=-1, more=(), **kw):
        with step_clip.StepClip() as clip:
            got = clip.open_checked([(path, "color_video", missing)] + list(more), decoder, encoder,
                                    lambda n: step_clip.frames_to_write(n, max_frames), **kw)
            return clip, got
    # each refusal with everything after it wrong as well: the earlier one wins
    with pytest.raises(Exception) as e:
        host_phase(str(tmp_path / "gone.npy"), "device", "device", 0)
    assert e.value is missing and sorted(os.listdir(tmp_path)) == before
    for args, text in (((planes, "device", "device", 0), "--video_decoder device decodes .mkv inputs: a .npy input is a raw frame dump"),
                       ((planes, "host", "device", 0), "--video_encoder device encodes .mkv outputs"),
                       ((planes, "host", "host", 0), planes + ": uint8 [N, H, W, 3] expected"),
                       ((frames, "host", "host", 0), "No frames read")):
        with pytest.raises(ValueError) as e:
            host_phase(*args)
        assert str(e.value).startswith(text) and sorted(os.listdir(tmp_path)) == before, text
    # what the tool reads off a clip that passes; the frame rate of a dump is None
    clip, (color,) = host_phase(frames, max_frames=2)
    assert (clip.video, clip.n, clip.H, clip.W, clip.fps) == (False, 2, 4, 5, None) and color.shape == (3, 4, 5, 3)
    # two inputs: the shorter one counts, each has its own exception, the label words the shape message
    short = str(tmp_path / "short.npy")
    np.save(short, np.zeros((2, 6, 7, 3), np.uint8))
    other = Exception("input depth_video does not exist")
    clip, _ = host_phase(frames, more=[(short, "depth_video", other)])
    assert (clip.n, clip.H, clip.W) == (2, 4, 5)
    with pytest.raises(Exception) as e:
        host_phase(frames, more=[(str(tmp_path / "gone.npy"), "depth_video", other)])
    assert e.value is other
    with pytest.raises(ValueError) as e:
        host_phase(frames, more=[(planes, "depth_video", other)], label="--{name}")
    assert str(e.value) == "--depth_video: uint8 [N, H, W, 3] expected"
    assert sorted(os.listdir(tmp_path)) == sorted(before + ["short.npy"])


def test_the_list_loop_keeps_its_order(tmp_path, capsys, monkeypatch):
    from metric_depth_video_toolbox_amd import step_clip
    lst, one = tmp_path / "clips.txt", tmp_path / "one.txt"
    lst.write_text("a.mkv\nb.mkv\nc.mkv\n")
    one.write_text("a.mkv\n")
    log = []
    real_read = step_clip.read_list_file

    def check(a):
        log.append("check")

    def load():
        log.append("load")
        return "the model"

    def run_clip(a, path, infer):
        log.append(("clip", path, infer))
        return path + "_out"

    def reading(path):
        log.append("read")
        return real_read(path)
    monkeypatch.setattr(step_clip, "read_list_file", reading)
    args = argparse.Namespace(color_video=str(lst))
    assert step_clip.run_list(args, None, check, load, run_clip) == ["a.mkv_out", "b.mkv_out", "c.mkv_out"]
    assert log == ["check", "read", "load"] + [("clip", p, "the model") for p in ("a.mkv", "b.mkv", "c.mkv")]      # loaded once
    assert capsys.readouterr().out == "".join(f"\n##### [{k}/3] Processing {p} #####\n" for k, p in enumerate(("a.mkv", "b.mkv", "c.mkv"), 1))
    # a generator that is handed in is not loaded; a list of one entry has its banner, a single clip has none
    del log[:]
    assert step_clip.run_list(argparse.Namespace(color_video=str(one)), "mine", check, load, run_clip, banner="\n##### [{k}/{n}] {path} #####") == ["a.mkv_out"]
    assert log == ["check", "read", ("clip", "a.mkv", "mine")] and capsys.readouterr().out == "\n##### [1/1] a.mkv #####\n"
    assert step_clip.run_list(argparse.Namespace(color_video="a.mkv"), "mine", check, load, run_clip) == ["a.mkv_out"]
    assert capsys.readouterr().out == ""
    # a failing flag check: nothing is read or loaded
    del log[:]

    def refusing(a):
        raise ValueError("--batch must be at least 1")
    with pytest.raises(ValueError, match="--batch"):
        step_clip.run_list(args, None, refusing, load, run_clip)
    assert log == []
    # a clip's exception propagates and the later clips do not run

    def second_fails(a, path, infer):
        log.append(path)
        if path == "b.mkv":
            raise RuntimeError("clip b failed")
        return path
    with pytest.raises(RuntimeError, match="clip b failed"):
        step_clip.run_list(args, "mine", check, load, second_fails)
    assert log == ["check", "read", "a.mkv", "b.mkv"]


def test_the_wrappers_argument_helpers_word_their_refusals():
    from metric_depth_video_toolbox_amd import step_clip
    assert step_clip.size_arg((7.0, "3"), "out_size") == (7, 3)
    for size, what in (((0, 3), "out_size"), ((3, -1), "model_size")):
        with pytest.raises(ValueError) as e:
            step_clip.size_arg(size, what)
        assert str(e.value) == f"{what} must be (width, height) with both at least 1, got {size!r}"
    t = np.zeros((2, 3, 4, 3), np.uint8)
    assert step_clip.non_empty("frames", t, "pixel") == (2, 3, 4) and step_clip.non_empty("points", t, "point", (2, 4, 3)) == (2, 4, 3)
    with pytest.raises(ValueError) as e:
        step_clip.non_empty("planes", np.zeros((2, 0, 4), np.float32), "value")
    assert str(e.value) == "planes holds no value: shape (2, 0, 4)"


def test_the_module_takes_no_tensors_address_and_imports_no_torch_at_the_top():
    src = open(os.path.join(REPO, "metric_depth_video_toolbox_amd", "step_clip.py")).read()
    assert "data_ptr" not in src
    assert not [ln for ln in src.splitlines() if ln.startswith(("import torch", "from torch"))]
