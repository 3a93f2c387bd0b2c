"""video_metric_convert's host side -- no GPU: the binding of the two entry points of include/mdvt_metric_align.h, NumPy's float32
order of summation pinned against a scalar model (the order csrc/mdvt_metric_align.hip reproduces through mdvt_pairwise.h), the
condition on the fit tests' inputs (they must tell that order from two others), the Python argument checks and the command line's
refusals, and the resize tables of tests/metric_align_ref.py."""
import os
import re

import numpy as np
import pytest

import metric_align_ref as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_entry_points_are_exported_outside_the_main_header():
    from metric_depth_video_toolbox_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "mdvt_metric_align.h")).read()
    declared = sorted(set(re.findall(r"\b(mdvt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))))
    assert declared == sorted(_lib.METRIC_ALIGN_SYMBOLS) == ["mdvt_metric_depth_codes", "mdvt_scale_shift_fit"]
    for s in _lib.METRIC_ALIGN_SYMBOLS:
        assert hasattr(L, s) and s not in _lib.SYMBOLS and s not in _lib.DECODE_SYMBOLS and s not in _lib.CONVERGENCE_SYMBOLS
    main = open(os.path.join(REPO, "include", "mdvt.h")).read()
    assert "mdvt_scale_shift_fit" not in main and "mdvt_metric_depth_codes" not in main
    assert L.mdvt_version() == 15                                   # ABI 0.15: include/mdvt.h is unchanged
    for doc in ("video_metric_convert.py:17-41", "depthcrafter_video.py:236-243", "RESTATED, not observed"):
        assert doc in hdr


SIZES = [1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 16384 + 5, 3 * 8192 + 1003]


@pytest.mark.parametrize("n", SIZES)
def test_numpy_sums_float32_in_chunks_of_8192_pairwise(n):
    """np.sum of a contiguous float32 array = chunks of 8192 / pw / in sequence, for the fit's five arrays, 1-D and [n_frames * H, W]."""
    assert np.getbufsize() == 8192
    rng = np.random.default_rng(n)
    p, d = mr.gen_spread(rng, 1, 1, n)
    m = mr.gen_mask(rng, 1, 1, n)
    for a in mr.five_arrays(p.ravel(), mr.inverse(d).ravel(), m.ravel()):
        want = np.sum(a)
        assert want.dtype == np.float32 and mr.sum_chunked(a).tobytes() == want.tobytes()
        for w in (1, 3, 7, 43):                                     # the same values as [rows, w]: a contiguous array sums like its flattening
            if n % w == 0:
                assert np.sum(a.reshape(n // w, w)).tobytes() == want.tobytes(), (n, w)


# every input the GPU fit tests draw (metric_align_ref.FIT_INPUTS: the same generator, shape and seed, so the same arrays)
TELLING = sorted({case for cases in mr.FIT_INPUTS.values() for case in cases})
BOTH_FROM = 32 * 96 * 172


@pytest.mark.parametrize("gen,shape,seed", TELLING, ids=[f"{g}-{'x'.join(map(str, s))}-{seed}" for g, s, seed in TELLING])
def test_the_fit_inputs_tell_the_orders_apart(gen, shape, seed):
    """Inputs on which NumPy's order, a left-to-right float32 sum and a float64 sum rounded once all agree in all five sums are not
    accepted, with and without the mask; from 32 x 96 x 172 values on NumPy's order must differ from each of the other two.  (A
    pairwise sum of one or two chunks is often the correctly rounded one, which is what the float64 sum gives: there only the
    left-to-right sum is told apart.)  Below 8 values NumPy's order is the left-to-right one, and nothing can tell them apart."""
    p, d, m = mr.fit_input(gen, shape, seed)
    n = p.size
    for mask in (None, mr.concat(m)):
        sequential, wide = mr.orders_told_apart(mr.concat(p), mr.concat(mr.inverse(d)), mask)
        if n < 8:
            assert not sequential
            continue
        assert sequential or wide, (gen, shape, mask is not None, sequential, wide)
        if n >= BOTH_FROM:
            assert sequential and wide, (gen, shape, mask is not None, sequential, wide)


def test_the_solve_and_its_degenerate_cases():
    one = mr.fit(np.array([[2.0]], F), np.array([[0.5]], F))
    assert one[7] == 0 and (one[5], one[6]) == (1, 0)               # one element: det = p^2 * 1 - p * p = 0
    zero = mr.fit(np.zeros((4, 5), F), np.ones((4, 5), F))
    assert zero[7] == 0 and (zero[5], zero[6]) == (1, 0)
    nan = mr.fit(np.array([[1.0, 2.0]], F), np.array([[np.inf, 1.0]], F))
    assert np.isnan(nan[5]) and np.isnan(nan[6])                    # a NaN det is != 0: the division runs
    p = np.array([[1.0, 2.0, 3.0, 4.0]], F)
    exact = mr.fit(p, p * F(0.5) + F(0.25))
    assert exact[5] == F(0.5) and exact[6] == F(0.25)


def test_python_argument_checks_come_before_any_device_call():
    torch = pytest.importorskip("torch")
    from metric_depth_video_toolbox_amd import video_metric_convert as vmc
    cpu = torch.zeros((2, 3, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="prediction must be a CUDA tensor"):
        vmc.compute_scale_and_shift_full(cpu, cpu)
    with pytest.raises(ValueError, match="prediction must be a CUDA tensor"):
        vmc.compute_scale_and_shift_full(np.zeros((3, 4), F), cpu)
    with pytest.raises(ValueError, match="max_depth"):
        vmc.metric_depth_codes(cpu, cpu, 0)
    with pytest.raises(ValueError, match="style"):
        vmc.metric_depth_codes(cpu, cpu, 100, style=2)
    with pytest.raises(ValueError, match="out_size"):
        vmc.metric_depth_codes(cpu, cpu, 100, out_size=(0, 5))
    with pytest.raises(ValueError, match="relative must be a CUDA tensor"):
        vmc.metric_depth_codes(cpu, cpu, 100)
    with pytest.raises(ValueError, match="engine"):
        vmc.convert(cpu, cpu, engine="midas")
    with pytest.raises(ValueError, match="engine"):
        vmc.fit_reference(cpu, cpu, engine="midas")
    with pytest.raises(ValueError, match="max_depth"):
        vmc.fit_reference(cpu, cpu, -1)


def test_cli_flags_and_refusals(tmp_path):
    from metric_depth_video_toolbox_amd import video_io, video_metric_convert as vmc
    p = vmc.build_parser()
    a = p.parse_args(["--color_video", "x.mkv", "--relative_depth", "r.npy", "--depth_video", "d.mkv"])
    assert (a.metric_depth, a.max_depth, a.max_frames, a.engine, a.batch, a.video_encoder, a.video_decoder) == \
        (None, 100, -1, "vda", 16, "host", "host")
    a = p.parse_args(["--color_video", "x.mkv", "--relative_depth", "r.npy", "--metric_depth", "m.npy", "--max_depth", "20", "--max_frames", "5",
                      "--engine", "depthcrafter", "--batch", "4", "--video_encoder", "device", "--video_decoder", "device"])
    assert (a.metric_depth, a.max_depth, a.max_frames, a.engine, a.batch, a.video_encoder, a.video_decoder) == \
        ("m.npy", 20, 5, "depthcrafter", 4, "device", "device")
    for bad in ([], ["--color_video", "x.mkv"], ["--color_video", "x.mkv", "--relative_depth", "r.npy", "--engine", "midas"],
                ["--color_video", "x.mkv", "--relative_depth", "r.npy", "--video_encoder", "gpu"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert vmc.output_paths("x.mkv") == ("x.mkv_tmp_depth.mkv", "x.mkv_depth.mkv")          # vmc:146-147

    color = str(tmp_path / "x.mkv")
    with video_io.VideoWriter(color, 16, 10, 25.0) as w:
        for _ in range(3):
            w.write(np.zeros((10, 16, 3), np.uint8))
    rel, ref, small, coded, f64 = (str(tmp_path / n) for n in ("rel.npy", "ref.npy", "small.npy", "coded.npy", "f64.npy"))
    np.save(rel, np.ones((3, 6, 8), F))
    np.save(ref, np.ones((3, 6, 8), F))
    np.save(small, np.ones((3, 5, 8), F))
    np.save(coded, np.zeros((3, 5, 8, 3), np.uint8))
    np.save(f64, np.ones((3, 6, 8), np.float64))
    with pytest.raises(ValueError, match="exactly one"):
        vmc.run(color, rel)
    with pytest.raises(ValueError, match="exactly one"):
        vmc.run(color, rel, coded, ref)
    with pytest.raises(FileNotFoundError, match="Color video"):
        vmc.run(str(tmp_path / "no.mkv"), rel, metric_depth=ref)
    with pytest.raises(FileNotFoundError, match="Relative depth"):
        vmc.run(color, str(tmp_path / "no.npy"), metric_depth=ref)
    with pytest.raises(FileNotFoundError, match="Reference depth"):
        vmc.run(color, rel, metric_depth=str(tmp_path / "no.npy"))
    with pytest.raises(ValueError, match="engine"):
        vmc.run(color, rel, metric_depth=ref, engine="midas")
    with pytest.raises(ValueError, match="max_depth"):
        vmc.run(color, rel, metric_depth=ref, max_depth=0)
    with pytest.raises(ValueError, match="video_encoder"):
        vmc.run(color, rel, metric_depth=ref, video_encoder="gpu")
    with pytest.raises(ValueError, match="video_decoder device"):
        vmc.run(color, rel, metric_depth=ref, video_decoder="device")    # a frame dump is not decoded
    with pytest.raises(ValueError, match="must be an .mkv"):
        vmc.run(rel, rel, metric_depth=ref)
    with pytest.raises(ValueError, match=r"float32 \[N, h, w\]"):
        vmc.run(color, f64, metric_depth=ref)
    with pytest.raises(ValueError, match=r"float32 \[N, h, w\]"):
        vmc.run(color, rel, metric_depth=f64)
    with pytest.raises(ValueError, match="does not resize reference frames"):
        vmc.run(color, rel, metric_depth=small)
    with pytest.raises(ValueError, match="does not resize reference frames"):
        vmc.run(color, rel, depth_video=coded)
    with pytest.raises(ValueError, match=r"uint8 \[N, H, W, 3\]"):
        vmc.run(color, rel, depth_video=ref)
    with pytest.raises(ValueError, match="no frame"):
        vmc.run(color, rel, metric_depth=ref, max_frames=0)
    assert sorted(os.listdir(tmp_path)) == ["coded.npy", "f64.npy", "ref.npy", "rel.npy", "small.npy", "x.mkv"]      # nothing was written


TABLES = [(1, 1), (1, 5), (5, 1), (7, 7), (17, 64), (64, 17), (924, 1920)]


@pytest.mark.parametrize("n_in,n_out", TABLES)
def test_resize_tables(n_in, n_out):
    s0, s1, w0, w1 = mr.linear_table(n_in, n_out)
    assert s0.min() >= 0 and s0.max() <= n_in - 1 and s1.min() >= 0 and s1.max() <= n_in - 1 and ((s1 == s0) | (s1 == s0 + 1)).all()
    assert w0.dtype == w1.dtype == np.float32
    assert (w0 >= 0).all() and (w0 <= 1).all() and (w1 >= 0).all() and (w1 <= 1).all()
    assert ((w1 == 0) | (s1 == s0 + 1)).all()                       # a weight on the second tap only where there is one
    if n_in == n_out:
        assert np.array_equal(s0, np.arange(n_in)) and (w0 == 1).all() and (w1 == 0).all()
    rng = np.random.default_rng(n_in * 4099 + n_out)
    d = rng.random((3, n_in), dtype=F)
    out = mr.resize_linear(d, n_out, 3)
    assert out.shape == (3, n_out) and out.dtype == np.float32
    eps = 2 * np.spacing(F(1))                                      # a convex combination, up to the roundings of 1 - f and of the sum
    assert out.min() >= d.min() - eps and out.max() <= d.max() + eps
    if n_in == n_out:
        assert out is d or np.array_equal(out, d)
    flat = np.full((4, n_in), F(0.7))
    assert (mr.resize_linear(flat, n_out, 9) - F(0.7)).max() <= np.spacing(F(0.7))


def test_the_code_is_the_existing_one():
    """dfh:5-11, 48-61 on a ramp: R = G = byte 3, B = byte 2 of trunc(255^4 / max_depth * depth)."""
    d = np.array([[0.0, 1e-6, 0.5, 1.0, 99.99999, 100.0, 250.0, -3.0]], F)
    c, rgb = mr.code(d, 100)
    assert c.tolist() == [[0.0, F(1e-6), 0.5, 1.0, F(99.99999), 100.0, 100.0, 0.0]]
    u = [int((255 ** 4 / 100.0) * float(v)) for v in c[0]]
    assert rgb[0, :, 0].tolist() == rgb[0, :, 1].tolist() == [v >> 24 for v in u] and rgb[0, :, 2].tolist() == [(v >> 16) & 255 for v in u]
    assert np.array_equal(mr.code(d, 100, bgr=True)[1], rgb[..., ::-1])
