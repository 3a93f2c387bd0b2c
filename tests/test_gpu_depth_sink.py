"""mdvt_depth_video_codes (include/mdvt_depth_sink.h) and its Python face in tools/video_da3.py against NumPy on the test machine
(tests/depth_sink_ref.py): the code bytes and the coded depth planes bit for bit -- the same 32 bits, or both NaN; no tolerance -- at
every width around the four-pixel groups, with and without a resize, on padded and gapped layouts, on the 16-byte load path and the
element path, with every value the sink can meet and every factor.

Which layouts take the 16-byte loads (the library does not report it; include/mdvt_depth_sink.h states it): no resize, and the plane's
address, pitch and stride multiples of 16.  The tests name the path each layout takes by that rule and insist that both are reached."""
import importlib.util
import os

import numpy as np
import pytest

import depth_sink_ref as dr
import metric_align_ref as mr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def mods():
    import torch
    from metric_depth_video_toolbox_amd import _lib
    spec = importlib.util.spec_from_file_location("video_da3_tool", os.path.join(REPO, "tools", "video_da3.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ctx = _lib.Context(0, 16, 16)
    yield torch, _lib, tool, ctx
    ctx.close()


SPECIALS = np.array([np.nan, np.inf, 3.5, -np.inf, 2.25, -1.5, -0.0, 0.0, 1e-40, 250.0, 19.999999, 7.0, 20.0, 100.0, 6.9999995], F)


def values(rng, N, h, w, max_depth, specials=True):
    """Depths in [0, 1.3 max_depth) with, every fifth value, one of SPECIALS: NaN and both infinities next to finite values, negatives,
    -0, a denormal, values above and at max_depth."""
    x = (rng.random((N, h, w), dtype=F) * F(1.3 * max_depth)).astype(F)
    if specials:
        flat = x.reshape(-1)
        flat[::5] = np.resize(SPECIALS, flat[::5].size)
    return x


def strided(torch, planes, pad, gap, base):
    """The planes inside a NaN-poisoned buffer: rows pad and frames gap values longer, `base` values past a 256-byte boundary."""
    planes = np.ascontiguousarray(planes, F)
    N, H, W = planes.shape
    pitch = W + pad
    stride = H * pitch + gap
    buf = torch.full((64 + base + N * stride + 64,), float("nan"), dtype=torch.float32, device="cuda")
    at = (-(buf.data_ptr() // 4)) % 64 + base
    view = torch.as_strided(buf, (N, H, W), (stride, pitch, 1), at)
    view.copy_(torch.from_numpy(planes).cuda())
    return view


def takes_vector_loads(t, resized):
    N, _, W = t.shape
    return (not resized) and W >= 4 and t.data_ptr() % 16 == 0 and (4 * t.stride(1)) % 16 == 0 and (N == 1 or (4 * t.stride(0)) % 16 == 0)


def check(mods, x, max_depth, out_size, *, scale=None, nan_to_max=False, bgr=False, plane=True, layout=(0, 0, 0), what=""):
    """One call on `x` laid out as `layout` = (pad, gap, base) against the restatement; -> whether it took the 16-byte loads."""
    torch, _lib, tool, ctx = mods
    t = strided(torch, x, *layout)
    d_scale = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
    got = tool.depth_video_codes(ctx, t, max_depth, out_size, scale=d_scale, nan_to_max=nan_to_max, bgr=bgr, want_plane=plane)
    codes, planes = (got[0], got[1]) if plane else (got, None)
    want_codes, want_planes = dr.sink(x, max_depth, out_size, scale, nan_to_max, bgr)
    codes = codes.cpu().numpy()
    bad = np.argwhere((codes != want_codes).any(-1))
    print(f"{what}: {len(bad)} of {want_codes[..., 0].size} codes differ")
    assert bad.size == 0, f"{what}: first at (frame, row, column) {tuple(bad[0])}: got {codes[tuple(bad[0])]}, want {want_codes[tuple(bad[0])]}"
    if plane:
        off = mr.same_bits(planes.cpu().numpy(), want_planes)
        assert off.size == 0, f"{what}: {off.size} plane values differ, first at {off[0]}"
    resized = out_size is not None and tuple(out_size) != (x.shape[2], x.shape[1])
    return takes_vector_loads(t, resized)


def test_every_width_around_a_group_of_four(mods):
    """out_w 1 .. 9 from sources of 1 and 2 values per axis (the clamped taps) and from a source of the same size."""
    rng = np.random.default_rng(171)
    k = 0
    for ow in (1, 2, 3, 4, 5, 7, 8, 9):
        for iw in (1, 2):
            for ih in (1, 2):
                k += 1
                x = values(rng, 2, ih, iw, 20, specials=k % 2 == 0)
                check(mods, x, 20, (ow, 3), bgr=bool(k % 2), scale=None if k % 3 else 0.75, what=f"{iw}x{ih} -> {ow}x3")
        x = values(rng, 2, 3, ow, 20)
        check(mods, x, 20, (ow, 3), nan_to_max=bool(ow % 2), layout=(0, 0, 0), what=f"{ow}x3 as it is")
        check(mods, x, 20, None, nan_to_max=bool(ow % 2), layout=(1, 3, 1), what=f"{ow}x3 as it is, odd layout")


# (in_w, in_h) -> (out_w, out_h): no resize; the vector stores behind a resize; down; one value up; a ratio that is no integer
SIZES = [((37, 23), (37, 23)), ((36, 20), (36, 20)), ((36, 20), (64, 36)), ((7, 5), (3, 2)), ((1, 1), (5, 4)), ((21, 12), (80, 45))]
# (pad, gap, base) in values: dense and aligned; padded pitches and gapped strides, 16-byte multiples; the base 4 values on; 1 value on
LAYOUTS = [(0, 0, 0), (4, 8, 0), (4, 8, 4), (3, 5, 1)]
_reached = {}


@pytest.mark.parametrize("size", SIZES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES])
def test_codes_and_planes_equal_numpy(mods, size):
    """3 frames; both orders, with and without the factor, the NaN rule and the plane output; max_depth 7, 20 and 100."""
    (w, h), out = size
    rng = np.random.default_rng(w * 100 + out[0])
    k = 0
    for layout in LAYOUTS:
        for max_depth in (7, 20, 100):
            k += 1
            x = values(rng, 3, h, w, max_depth)
            vec = check(mods, x, max_depth, out, scale=(None, 1.2345678, 0.4)[k % 3], nan_to_max=bool(k % 2), bgr=bool((k // 2) % 2),
                        plane=k % 4 != 3, layout=layout, what=f"{w}x{h} -> {out[0]}x{out[1]} layout {layout} max_depth {max_depth}")
            if (w, h) == out:
                _reached.setdefault((w, h), set()).add((layout, vec))
    if (w, h) == (36, 20):                                           # the plan: both load paths ran, by the header's rule
        assert {v for _, v in _reached[(36, 20)]} == {True, False}
        assert ((4, 8, 4), True) in _reached[(36, 20)] and ((3, 5, 1), False) in _reached[(36, 20)]
    if (w, h) == (37, 23):                                           # an odd width: padded by 3 values the pitch is a multiple of 16 again
        assert ((0, 0, 0), False) in _reached[(37, 23)] and ((3, 5, 1), False) in _reached[(37, 23)]


def test_both_load_paths_give_the_same_bits(mods):
    torch, _lib, tool, ctx = mods
    x = values(np.random.default_rng(5), 3, 20, 36, 20)
    outs = []
    for layout in ((4, 8, 4), (3, 5, 1)):
        t = strided(torch, x, *layout)
        codes, plane = tool.depth_video_codes(ctx, t, 20, None, want_plane=True)
        outs.append((takes_vector_loads(t, False), codes.cpu().numpy(), plane.cpu().numpy()))
    assert [o[0] for o in outs] == [True, False]
    assert np.array_equal(outs[0][1], outs[1][1]) and mr.same_bits(outs[0][2], outs[1][2]).size == 0


@pytest.mark.parametrize("s", [0.0, 2.0 ** -130, 1.2345678, np.inf, np.nan], ids=["0", "2^-130", "1.2345678", "inf", "nan"])
def test_every_factor(mods, s):
    rng = np.random.default_rng(9)
    for (w, h), out in (((37, 23), (37, 23)), ((21, 12), (80, 45))):
        x = values(rng, 2, h, w, 20)
        check(mods, x, 20, out, scale=s, nan_to_max=True, what=f"factor {s!r} {w}x{h} -> {out[0]}x{out[1]}")
        check(mods, x, 20, out, scale=s, nan_to_max=False, layout=(3, 5, 1), what=f"factor {s!r} {w}x{h} -> {out[0]}x{out[1]} NaN kept")


def test_fit_and_sink_on_one_stream_without_a_read_back(mods):
    """The batch factor goes from the fit's sums to the sink on the device: s is fit's b_0 / max(a_00, 1e-12) bit for bit."""
    torch, _lib, tool, ctx = mods
    rng = np.random.default_rng(31)
    earlier = values(rng, 5, 12, 21, 20, specials=False) + F(0.25)
    again = (earlier * F(1.0 / 1.37) + rng.normal(0, 0.01, earlier.shape).astype(F)).astype(F)
    new = values(rng, 3, 12, 21, 20)
    v = mr.fit(mr.concat(again), mr.concat(earlier))
    want_s = F(v[3] / np.maximum(v[0], F(1e-12)))
    assert want_s == dr.batch_scale(earlier, again) and 1.3 < want_s < 1.45
    side = torch.cuda.Stream()
    d_earlier, d_again, d_new = (torch.from_numpy(a).cuda() for a in (earlier, again, new))
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = tool.batch_scale(d_earlier, d_again)
        codes, plane = tool.depth_video_codes(ctx, d_new, 20, (80, 45), scale=s, want_plane=True)
    side.synchronize()
    assert s.dtype == torch.float32 and s.numel() == 1 and s.cpu().numpy()[0].tobytes() == want_s.tobytes()
    want_codes, want_plane = dr.sink(new, 20, (80, 45), want_s)
    assert np.array_equal(codes.cpu().numpy(), want_codes) and mr.same_bits(plane.cpu().numpy(), want_plane).size == 0
    # a sum of 0 takes the floor
    zero = torch.zeros((1, 4, 4), device="cuda")
    assert tool.batch_scale(d_earlier[:1, :4, :4].contiguous(), zero).item() == 0.0


def test_one_full_size_case(mods):
    x = values(np.random.default_rng(1080), 2, 280, 504, 100)
    check(mods, x, 100, (1920, 1080), scale=0.987654, what="504x280 -> 1920x1080")


def test_the_python_face_refuses_what_the_contract_excludes(mods):
    torch, _lib, tool, ctx = mods
    x = torch.ones((2, 5, 8), device="cuda")
    with pytest.raises(TypeError):
        tool.depth_video_codes(ctx, x.double(), 20)
    with pytest.raises(ValueError):
        tool.depth_video_codes(ctx, x.cpu(), 20)
    with pytest.raises(ValueError):
        tool.depth_video_codes(ctx, x[:, :, ::2], 20)               # a column stride
    with pytest.raises(ValueError):
        tool.depth_video_codes(ctx, x, 0)
    with pytest.raises(ValueError):
        tool.depth_video_codes(ctx, x, 20, scale=torch.ones(2, device="cuda"))
    with pytest.raises(TypeError):
        tool.depth_video_codes(ctx, x, 20, scale=1.5)
    with pytest.raises(ValueError):
        tool.depth_video_codes(ctx, x, 20, out=torch.empty((2, 5, 9, 3), dtype=torch.uint8, device="cuda"))
    out = torch.empty((2, 5, 8, 3), dtype=torch.uint8, device="cuda")
    assert tool.depth_video_codes(ctx, x, 20, out=out) is out and int(out[0, 0, 0, 0]) == int(255 / 20)


def test_save_depth_video_writes_the_sinks_frames(mods, tmp_path):
    """The sink alone, for any metric model: planes -> .mkv, read back and compared; the device encoder gives the same file."""
    torch, _lib, tool, ctx = mods
    from metric_depth_video_toolbox_amd.clip_io import open_frames
    x = values(np.random.default_rng(12), 5, 8, 12, 20)
    want = dr.sink(x, 20, (48, 32), None, True)[0]
    files = []
    for enc in ("host", "device"):
        path = str(tmp_path / f"depth_{enc}.mkv")
        tool.save_depth_video(torch.from_numpy(x).cuda(), path, 24.0, 20, 48, 32, nan_to_max=True, video_encoder=enc, batch=2)
        frames = open_frames(path, FileNotFoundError(path))
        assert np.array_equal(np.array(frames[0:5]), want), enc
        frames.close()
        files.append(open(path, "rb").read())
    assert files[0] == files[1]
