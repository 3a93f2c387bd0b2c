"""No GPU needed: the table of tests/binding_contract.py is in step with the package's sources -- a new wrapper that hands a tensor's
address to the library needs a record before this passes -- and its extent checker catches the slips it is there to catch, on
hand-made recordings over host tensors."""
import glob
import os
import subprocess
import sys

import pytest

import binding_contract as bc

PKG_DIR = os.path.join(bc.REPO, bc.PKG)

# entry points a covered module reaches that take no tensor of a caller's (host arithmetic, parsers of host bytes, context settings)
NO_TENSOR = {"mdvt_equirect_tables": "host tables into NumPy arrays the wrapper allocates",
             "mdvt_ffv1_decode_supported": "parses a configuration record (host bytes)",
             "mdvt_ffv1_stream_decode_supported": "parses a configuration record (host bytes)",
             "mdvt_ffv1_packet_is_key": "reads a packet's first bit (host bytes)",
             "mdvt_set_config": "a configuration record, no buffer", "mdvt_set_near_clip": "a switch, no buffer"}


def _source(module):
    with open(os.path.join(PKG_DIR, module + ".py")) as f:
        return f.read()


def test_every_site_that_takes_a_tensors_address_has_a_record():
    sites = bc.package_sites()
    assert len(sites) >= 50 and "stereo_rerender.StereoRerenderer.prepare" in sites and "depth_frames_helper.swap_rb" in sites
    covered = {s for r in bc.RECORDS for s in r.sites}
    missing = sorted(set(sites) - covered)
    assert not missing, f"functions that take a tensor's data_ptr() without a record in tests/binding_contract.py: {missing}"
    stale = sorted(covered - set(sites))
    assert not stale, f"sites named in tests/binding_contract.py that take no data_ptr() in the package's sources: {stale}"
    outside = sorted({fn[:-3] for fn in sites.values()} - set(bc.MODULES))
    assert not outside, f"modules that take a tensor's address but are not listed in binding_contract.MODULES: {outside}"
    # every entry point the covered modules call -- through Context.call or bound directly, as PreparedRender binds
    # mdvt_render_stereo_batch -- has a pointer group in some record (or takes no tensor)
    grouped = {g.entry for r in bc.RECORDS for g in r.groups}
    for module in bc.MODULES:
        src = _source(module)
        named = bc.call_entries(src) | bc.bound_entries(src)
        missing = sorted(named - grouped - set(NO_TENSOR))
        assert not missing, f"{module}.py reaches {missing}: no record of tests/binding_contract.py has a pointer group for it"
    assert "mdvt_render_stereo_batch" in bc.bound_entries(_source("stereo_rerender"))
    assert not set(NO_TENSOR) & grouped
    names = [r.name for r in bc.RECORDS]
    assert len(set(names)) == len(names)


def test_no_tool_outside_the_benchmarks_takes_a_tensors_address():
    """The benchmarks call the raw C ABI next to their yardsticks; every other tool reaches the library through the package."""
    tools = sorted(glob.glob(os.path.join(bc.REPO, "tools", "*.py")))
    assert len(tools) >= 10
    found = {}
    for path in tools:
        if not path.endswith("_bench.py"):
            with open(path) as f:
                found.update({s: os.path.basename(path) for s in bc.pointer_sites(f.read(), os.path.basename(path)[:-3])})
    assert not found, (f"tools that take a tensor's data_ptr(): {found}.  A wrapper that hands a tensor's address to the library belongs in the "
                       f"package (step_device.py, or a module of its step's own listed in binding_contract.MODULES) with a record in "
                       f"tests/binding_contract.py; the tool imports it from there")


def test_the_wrapper_modules_import_without_torch():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from metric_depth_video_toolbox_amd import step_device, megasam_device, inspatio_device; "
            "print('torch' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code, bc.REPO], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stderr[-2000:]


def test_a_record_of_frame_pairs_is_never_built_with_one_frame():
    """min_frames: the mid_frame layout (a batch of one frame) is left to the arguments that have no frame dimension."""
    assert "mid_frame" not in bc.layouts_of(bc.BY_NAME["step_device.frame_sums[no prev]"])
    r = bc.BY_NAME["step_device.frame_sums[prev]"]
    assert r.min_frames == 2 and "mid_frame" in bc.layouts_of(r)
    assert bc.Buffer._geometry(r.arg("frames"), r.arg("frames").dims(bc.Env(8, 4, 2)), "mid_frame")[4] is False
    assert bc.Buffer._geometry(r.arg("prev"), r.arg("prev").dims(bc.Env(8, 4, 2)), "mid_frame")[4] is True
    assert all(x.min_frames == 1 for x in bc.RECORDS if "frame_sums" not in x.name)


def test_the_site_parser_sees_methods_nested_helpers_and_conditional_names():
    src = '''
import x
def plain(t):
    return lib.call("mdvt_a", t.data_ptr())
def clean(t):
    return t.shape
class K:
    def method(self, t):
        def inner(u):
            self.ctx.call("mdvt_b" if u else "mdvt_c", u.data_ptr())
        inner(t)
    def other(self):
        return self._L.mdvt_d
'''
    assert bc.pointer_sites(src, "m") == {"m.plain", "m.K.method"}
    assert bc.call_entries(src) == {"mdvt_a", "mdvt_b", "mdvt_c"}
    assert bc.bound_entries(src) == {"mdvt_d"}


# tensor arguments whose address never reaches the library
UNGROUPED = {("stereo_rerender.infill_using_mask_normals", "img"): "copied into `out` by torch; the library fills `out` in place"}


def test_every_record_names_its_tensors_and_groups_consistently():
    for r in bc.RECORDS:
        names = [a.name for a in r.args]
        assert len(set(names)) == len(names) and r.groups, r.name
        for a in r.args:
            assert a.kind in ("rgb", "plane", "planar", "vec") and a.role in ("in", "out") and a.layout in ("strided", "contiguous", "copied"), (r.name, a.name)
            assert a.kind != "vec" or (a.layout == "contiguous" and a.shape is not None), (r.name, a.name)
            if (r.name, a.name) not in UNGROUPED:
                assert a.name in {g.arg for g in r.groups}, f"{r.name}: argument {a.name} has no pointer group"
        if r.inplace:
            assert set(r.inplace) <= set(names)
        assert "contiguous" in bc.layouts_of(r)
    by_layout = {lay: [r.name for r in bc.RECORDS if lay in bc.layouts_of(r)] for lay in bc.LAYOUTS}
    assert all(by_layout[lay] for lay in bc.LAYOUTS), by_layout
    assert sorted(by_layout["inplace"]) == ["depth_frames_helper.swap_rb", "stereo_rerender.infill_using_mask_normals"]


# ---- the extent checker on hand-made recordings ------------------------------------------------------------------------------------
W, H, N = 7, 4, 3


def _touch(t, **kw):
    """The right recording of a packed-pixel tensor [N,H,W,C] (or [H,W,C]): its own pointer, strides in bytes and sizes."""
    e = t.element_size()
    batched = t.dim() == 4
    d = dict(ptr=t.data_ptr(), pitch=t.stride(-3) * e, stride=t.stride(0) * e if batched else 0, n=int(t.shape[0]) if batched else 1,
             row_bytes=int(t.shape[-2]) * int(t.shape[-1]) * e, rows=int(t.shape[-3]))
    d.update(kw)
    return bc.Touch(**d)


def _planar_touch(t, **kw):
    """The right recording of a planar tensor [N, 3, H, W] (or [3, H, W]): its pointer and its three byte distances."""
    e = t.element_size()
    batched = t.dim() == 4
    d = dict(ptr=t.data_ptr(), pitch=t.stride(-2) * e, plane=t.stride(-3) * e, planes=int(t.shape[-3]), stride=t.stride(0) * e if batched else 0,
             n=int(t.shape[0]) if batched else 1, row_bytes=int(t.shape[-1]) * e, rows=int(t.shape[-2]))
    d.update(kw)
    return bc.Touch(**d)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def test_owned_bytes_of_views(torch):
    base = torch.zeros((N, H, 2 * W, 3), dtype=torch.uint8)
    p = base.data_ptr()
    assert list(bc.owned_bytes(base)) == list(range(p, p + base.numel()))
    right = base[:, :, W:]
    own = bc.owned_bytes(right)
    assert own.size == N * H * W * 3 and own[0] == p + 3 * W and own[-1] == p + base.numel() - 1
    assert own[3 * W] == p + 6 * W + 3 * W                                # the second row starts a whole side-by-side row on
    f = torch.zeros((H, W), dtype=torch.float32)
    assert bc.owned_bytes(f).size == 4 * H * W and bc.owned_bytes(f[:, ::2]).size == 4 * H * 4
    assert bc.owned_bytes(base[:1].expand(N, H, 2 * W, 3)).size == H * 2 * W * 3


def test_a_correct_recording_passes(torch):
    sbs = torch.zeros((N, H, 2 * W, 3), dtype=torch.uint8)
    for view in (sbs, sbs[:, :, W:], sbs[:, :, :W], sbs[1], sbs[::2], sbs[1:2], sbs[:1].expand(N, H, 2 * W, 3)[:, :, W:]):
        for output in (False, True):
            if output and view.stride(0) == 0:
                continue
            assert bc.check_groups("ok", view, [_touch(view)], output) == [], tuple(view.stride())
    # both eyes of a side-by-side buffer as two groups of one tensor
    both = [_touch(sbs, row_bytes=3 * W), _touch(sbs, ptr=sbs.data_ptr() + 3 * W, row_bytes=3 * W)]
    assert bc.check_groups("ok", sbs, both, True) == []
    z = torch.zeros((N, H, W, 1), dtype=torch.float32)
    assert bc.check_groups("ok", z, [_touch(z)], True) == []
    padded = torch.zeros((N, H, W + 5, 1), dtype=torch.float32)[:, :, :W]
    assert bc.check_groups("ok", padded, [_touch(padded)], True) == []
    # a planar tensor [N, 3, H, W] has a plane level: contiguous, with padded rows, and a slice of a ring of model frames
    ring = torch.zeros((5, 3, H, W + 5), dtype=torch.float32)
    for view in (ring, ring[:, :, :, :W], ring[1:1 + N], ring[1:1 + N, :, :, :W], ring[2]):
        for output in (False, True):
            assert bc.check_groups("ok", view, [_planar_touch(view)], output) == [], tuple(view.stride())


def test_the_slips_the_checker_exists_for_are_reported(torch):
    sbs = torch.zeros((N, H, 2 * W, 3), dtype=torch.uint8)
    right = sbs[:, :, W:]
    z = torch.zeros((N, H, W, 1), dtype=torch.float32)
    gapped = torch.zeros((N, H * W * 3 + 11), dtype=torch.uint8)[:, :H * W * 3].view(N, H, W, 3)
    planar = torch.zeros((5, 3, H, W), dtype=torch.float32)[1:1 + N]
    padded_planar = torch.zeros((5, 3, H, W + 5), dtype=torch.float32)[1:1 + N, :, :, :W]
    slips = {
        # an element stride where bytes are wanted, float32: pitch W instead of 4 W -- as an input (nothing out of bounds: part of
        # the tensor would be read four times over) and as an output
        "element stride for bytes, float32 input": (z, [_touch(z, pitch=W, stride=H * W)], False, "would not be read"),
        "element stride for bytes, float32 output": (z, [_touch(z, pitch=W, stride=H * W)], True, "would not be written"),
        # the contiguous pitch 3 W for a view whose rows are 6 W apart
        "contiguous pitch for one eye": (right, [_touch(right, pitch=3 * W, stride=3 * W * H)], True, "does not own"),
        "contiguous pitch for one eye, input": (right, [_touch(right, pitch=3 * W, stride=3 * W * H)], False, "does not own"),
        # the right eye's group without its + 3 W
        "missing eye offset": (sbs, [_touch(sbs, row_bytes=3 * W), _touch(sbs, row_bytes=3 * W)], True, "would not be written"),
        "missing eye offset on a view": (right, [_touch(right, ptr=sbs.data_ptr())], False, "does not own"),
        # n larger than the tensor's frame count
        "n beyond the frames": (sbs[:2], [_touch(sbs[:2], n=3)], True, "does not own"),
        "n beyond the frames, input": (sbs[:2], [_touch(sbs[:2], n=3)], False, "does not own"),
        # the frame stride of a contiguous batch for a gapped one
        "contiguous frame stride for a gapped batch": (gapped, [_touch(gapped, stride=3 * W * H)], True, "would not be written"),
        "contiguous frame stride for a gapped batch, input": (gapped, [_touch(gapped, stride=3 * W * H)], False, "would not be read"),
        # rows that fold onto one another in an output
        "folded rows": (sbs[0, :, :W], [_touch(sbs[0, :, :W], pitch=3 * W - 2)], True, "more than once"),
        # an element stride where the plane's byte distance is wanted: H W instead of 4 H W, on out=ring[at:at + k] of the MVSA ring
        "element stride for the plane distance, input": (planar, [_planar_touch(planar, plane=planar.stride(1))], False, "would not be read"),
        "element stride for the plane distance, output": (planar, [_planar_touch(planar, plane=planar.stride(1))], True, "would not be written"),
        # the contiguous plane distance for a view with padded rows
        "contiguous plane distance for padded rows": (padded_planar, [_planar_touch(padded_planar, plane=4 * H * W)], True, "does not own"),
    }
    for name, (tensor, touches, output, text) in slips.items():
        problems = bc.check_groups(name, tensor, touches, output)
        assert problems and any(text in p for p in problems), f"the slip '{name}' goes unnoticed: {problems}"
    # a last row that ends inside the storage but outside the view is named by frame, row and byte
    text = bc.check_groups("t", right, [_touch(right, pitch=3 * W, stride=3 * W * H)], True)[0]
    assert "(frame 0, row 1, byte 0)" in text and "pitch 21" in text, text
    text = bc.check_groups("t", padded_planar, [_planar_touch(padded_planar, plane=4 * H * W)], True)[0]
    # (plane 1 is told to start 4 H W = 112 bytes in: 16 bytes into the view's third row, which owns 12 more)
    assert "(frame 0, plane 1, row 0, byte 12)" in text and f"3 planes {4 * H * W} apart" in text, text
    assert bc.check_groups("none", sbs, [], True) == ["none: no pointer group was recorded"]
    # `partial` excuses unread bytes, never stray ones
    assert bc.check_groups("p", sbs, [_touch(sbs, row_bytes=3 * W)], False, partial=True) == []
    assert bc.check_groups("p", sbs[:2], [_touch(sbs[:2], n=3)], False, partial=True)


def test_the_recorder_stores_and_launches_nothing(torch):
    import ctypes as C
    _lib = bc.mod("_lib")
    before = (_lib.Context.call, _lib.SharedContext.call)
    ctx = object.__new__(_lib.SharedContext)                              # no device: the recorder never looks at the context
    io = _lib.MdvtIO()
    io.left_rgb, io.rgb_pitch = 4096, 18
    with bc.Recorder() as rec:
        ctx.call("mdvt_swap_rb", 1234, 21, 0, C.c_void_p(99), 21, 0, 1, C.c_void_p(None))
        _lib.Context.call(ctx, "mdvt_render_stereo_batch", 2, None, C.byref(io), None)
    assert (_lib.Context.call, _lib.SharedContext.call) == before
    assert [c.name for c in rec.calls] == ["mdvt_swap_rb", "mdvt_render_stereo_batch"]
    assert rec.calls[0].args == [1234, 21, 0, 99, 21, 0, 1, 0]
    assert rec.calls[1].args[2]["left_rgb"] == 4096 and rec.calls[1].args[2]["rgb_pitch"] == 18 and rec.calls[1].args[2]["right_rgb"] is None
    env = bc.Env(W, H)
    record = bc.BY_NAME["depth_frames_helper.swap_rb"]
    t = torch.zeros((N, H, 2 * W, 3), dtype=torch.uint8)[:, :, W:]
    call = bc.Call("mdvt_swap_rb", [t.data_ptr(), t.stride(1), t.stride(0), t.data_ptr(), t.stride(1), t.stride(0), N, 0])
    touched = bc.touches_of(record, [call], env)
    assert bc.check_groups("frames", t, touched["frames"], False) == [] and bc.check_groups("out", t, touched["out"], True) == []
    call.args[1] = 3 * W
    assert bc.check_groups("frames", t, bc.touches_of(record, [call], env)["frames"], False)


def test_check_tensor_refuses_by_raising(torch):
    """_lib.check_tensor on what needs no GPU: the dtype is a TypeError, the device a ValueError, each naming the argument."""
    _lib = bc.mod("_lib")
    t = torch.zeros((H, W, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="frames must be torch.uint8, got torch.float32"):
        _lib.check_tensor("frames", t.float(), torch.uint8)
    with pytest.raises(TypeError, match="frames must be a torch.Tensor"):
        _lib.check_tensor("frames", t.numpy(), torch.uint8)
    with pytest.raises(ValueError, match="frames must be on a GPU"):
        _lib.check_tensor("frames", t, torch.uint8)
