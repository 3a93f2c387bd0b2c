"""Every Python entry point that hands a tensor's address to the library, held to its tensor contract (tests/binding_contract.py has
the table, the recorder and the extent checker), in three passes kept apart:

  (a) refusals -- a tensor the docstring does not promise to take (wrong dtype, device, size or frame count, unpacked or transposed
      pixels, a strided tensor where no pitch is passed on, an output whose elements overlap) raises TypeError / ValueError before
      the recorder sees a call.  Nothing is launched: a missing check is a failed test, never a kernel on a bad address.
  (b) geometry -- for every layout the docstring accepts the call is recorded and every (pointer, pitch, stride, count) group is held
      to the tensor's own bytes.  Nothing is launched.
  (c) results -- only for a layout that passed (b) in this same run: the call is launched on views whose padding and gaps are
      poisoned; what is read through the views equals, byte for byte, the same function's result on contiguous copies with out=None
      (which the other GPU tests pin to the oracle), the padding and gaps of the outputs and all of the inputs are unchanged.  A
      layout that failed (b) is reported as failed here, without a launch.

Sizes: 33 x 5 (odd, across a 32-pixel word of the packed mask), 36 x 6 (a multiple of 4: the vector paths), 6 x 6 (square: a
transposed view keeps its shape), 3 frames; the model-sized buffers of the adapter and m2svid steps are 8 x 6 and 4 x 3.  The
model-step wrappers of step_device.py take the same: every size the clip does not fix differs from W x H -- the model's input and
PromptDA's prompt 8 x 6, MVSAnywhere's cost volume and its mask 4 x 3, the video a depth or a mask is resized to 9 x 7 -- and the
planar tensors [N, 3, h, w] bring a third byte distance, the plane's.  geometry_device.py's wrappers read W x H from the context,
so theirs is made for the frames' size.  The scene, tracker and InSpatio wrappers (step_device.frame_sums, megasam_device.py,
inspatio_device.py) take the same sizes, with these differences.  Passes (b) and (c) run the shift grid and InSpatio's compositing at
33 x 9, 36 x 12 and 8 x 8 (their entry points refuse an eye below 8 x 8), and cv2's area resize to 8 x 6 at 33 x 9, 36 x 10 and
10 x 10 (it refuses a frame smaller than 8 x 6 on an axis, and two integer ratios).  The tracker's inputs are cropped to 4 x 3 of its
8 x 6, its outputs go to the video's 9 x 7.  frame_sums compares pairs: its records are never built with fewer than two frames.
Every comparison is equality of bytes (floats: the same bits, or both NaN)."""
import pytest

import binding_contract as bc

pytestmark = pytest.mark.gpu

RECORD_NAMES = [r.name for r in bc.RECORDS]
GEOMETRY = {}                                # (record, W, H, layout, alt dtypes) -> problems of pass (b), shared with pass (c)


@pytest.fixture(scope="module")
def torch():
    import torch
    yield torch
    bc.close_renderers()


def _envs(record, layout, sizes=None):
    for W, H in (sizes or record.sizes):
        yield bc.make_env(record, W, H, layout)


def _variants(record):
    """(layout, alt dtypes): every layout the record's docstring accepts, and -- where an argument may come in a second dtype (a bool
    mask) -- that dtype once contiguous and once with padded rows."""
    out = [(layout, False) for layout in bc.layouts_of(record)]
    if any(a.also for a in record.args):
        out += [("contiguous", True)] + ([("row_pad", True)] if "row_pad" in bc.layouts_of(record) else [])
    return out


def _geometry(record, env, layout, alt):
    key = (record.name, env.W, env.H, layout, alt)
    if key not in GEOMETRY:
        GEOMETRY[key] = bc.geometry_problems(record, env, layout, alt_dtypes=alt)
    return GEOMETRY[key]


@pytest.mark.parametrize("name", RECORD_NAMES)
def test_a_refusals(torch, name):
    """Pass (a).  The other-GPU cases are there on a box with two GPUs only (binding_contract.refusal_cases)."""
    record = bc.BY_NAME[name]
    problems, cases = [], 0
    # 33 x 5 for everything; 6 x 6 adds the transposed square view
    for env in _envs(record, "contiguous", sizes=((33, 5), (6, 6))):
        cases += sum(len(bc.refusal_cases(record, a, env)) for a in record.args)
        problems += bc.refusal_problems(record, env)
    assert cases >= 3 * len(record.args)
    assert not problems, f"{len(problems)} of {cases} bad tensors were not refused before a library call:\n" + "\n".join(problems)


@pytest.mark.parametrize("name", RECORD_NAMES)
def test_b_geometry(torch, name):
    """Pass (b)."""
    record = bc.BY_NAME[name]
    problems = []
    for layout, alt in _variants(record):
        for env in _envs(record, layout):
            problems += _geometry(record, env, layout, alt)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", RECORD_NAMES)
def test_c_results(torch, name):
    """Pass (c)."""
    record = bc.BY_NAME[name]
    problems = []
    for layout, alt in _variants(record):
        for env in _envs(record, layout):
            bad = _geometry(record, env, layout, alt)
            if bad:
                problems.append(f"{name} [{layout}, {env.W}x{env.H}]: not launched, its geometry failed pass (b): {bad[0]}")
                continue
            problems += bc.result_problems(record, env, layout, alt_dtypes=alt)
    torch.cuda.synchronize()
    assert not problems, "\n".join(problems)


def test_a_missing_group_or_a_kept_assert_would_show(torch):
    """The passes on a wrapper made wrong on purpose: swap_rb told the contiguous pitch of its view fails (b), a wrapper that refuses
    with `assert` fails (a) -- both recorded only, never launched; a result off by one and a byte changed in front of the view
    (by torch, in the test's own buffer) fail (c)."""
    dfh = bc.mod("depth_frames_helper")
    record = bc.BY_NAME["depth_frames_helper.swap_rb"]

    def contiguous_pitch(e, a):
        f, o = a["frames"], a["out"]
        bc.mod("_lib").shared_context(f.device).call("mdvt_swap_rb", f.data_ptr(), 3 * e.W, 3 * e.W * e.H, o.data_ptr(), o.stride(-3), o.stride(0),
                                                     e.N, None)
        return {"out": o}

    def asserting(e, a):
        assert a["frames"].dtype == torch.uint8 and a["frames"].is_cuda and a["out"].is_cuda and a["out"].dtype == torch.uint8
        assert a["frames"].shape == a["out"].shape and a["frames"].stride(-1) == 1 and a["out"].stride(-2) == 3
        return {"out": dfh.swap_rb(a["frames"], out=a["out"])}
    env = bc.Env(33, 5)
    wrong = bc.Record("wrong", (), record.args, contiguous_pitch, record.groups)
    assert bc.geometry_problems(wrong, env, "contiguous") == []
    problems = bc.geometry_problems(wrong, env, "sbs_right")
    assert problems and all(" frames" in p for p in problems) and any("does not own" in p for p in problems), problems
    kept = bc.Record("kept", (), record.args, asserting, record.groups)
    text = "\n".join(bc.refusal_problems(kept, env))
    assert "refused by an assert" in text and "dtype int8" in text, text
    assert bc.refusal_problems(record, env) == []
    # pass (c) sees a result that differs and a byte written before the view (torch arithmetic on the test's own buffers)
    assert len(_variants(record)) >= 9 and len(_variants(bc.BY_NAME["stereo_rerender.infill_using_mask_normals"])) >= 11

    def off_by_one(e, a):
        out = dfh.swap_rb(a["frames"], out=a["out"])
        if a["out"] is not None:
            out.add_(1)
        return {"out": out}

    def stray(e, a):
        out = dfh.swap_rb(a["frames"], out=a["out"])
        if a["out"] is not None:
            out.as_strided((1,), (1,), out.storage_offset() - 1).add_(1)
        return {"out": out}
    env = bc.make_env(record, 33, 5, "row_pad")
    assert bc.result_problems(record, env, "row_pad") == []
    text = "\n".join(bc.result_problems(bc.Record("off", (), record.args, off_by_one, record.groups), env, "row_pad"))
    assert "result 'out' read through the view differs" in text, text
    text = "\n".join(bc.result_problems(bc.Record("stray", (), record.args, stray, record.groups), env, "row_pad"))
    assert "of the padding and gaps of output 'out' changed" in text and "differs" not in text, text
