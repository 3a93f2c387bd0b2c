"""bench.py --dump-outputs: what the timed path hands its caller goes to .npy files as float32 / float64, whole when small,
as exact per-frame sums plus a fixed, seeded pixel sample when large, under 64 MB either way (CPU tensors: no GPU needed)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402  (the repository root is on sys.path: tests/conftest.py)


def _outputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    sbs = torch.randint(0, 256, (N, H, 2 * W, 3), dtype=torch.uint8, generator=g)
    mask = torch.randint(0, 256, (N, H, 2 * W), dtype=torch.uint8, generator=g)
    return sbs, mask


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_dumped_whole(tmp_path):
    sbs, mask = _outputs(3, 20, 32, seed=1)
    bench.dump_outputs(str(tmp_path), sbs, mask, torch)
    got = _load(tmp_path)
    assert set(got) == {"sbs", "mask"}
    assert got["sbs"].dtype == np.float32 and np.array_equal(got["sbs"], sbs.numpy().astype(np.float32))
    assert got["mask"].dtype == np.float32 and np.array_equal(got["mask"], mask.numpy().astype(np.float32))


def test_large_outputs_are_summed_and_sampled_at_fixed_pixels(tmp_path):
    N, H, W = 4, 540, 960                                  # 16 B per sbs + mask pixel in float32: past DUMP_FULL_BYTES
    assert 16 * N * H * 2 * W > bench.DUMP_FULL_BYTES
    sbs, mask = _outputs(N, H, W, seed=2)
    for k, d in enumerate((tmp_path / "a", tmp_path / "b")):
        bench.dump_outputs(str(d), sbs, mask, torch, prefix="rank0_" if k else "")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"sbs_frame_sum", "mask_frame_sum", "sbs_sample", "mask_sample", "sample_frame_row_col"}
    assert set(b) == {"rank0_" + n for n in a}
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b["rank0_" + n])    # same pixels every time
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in a) <= 64 << 20
    s, m = sbs.numpy(), mask.numpy()
    assert np.array_equal(a["sbs_frame_sum"], s.reshape(N, -1, 3).sum(axis=1, dtype=np.int64).astype(np.float64))
    assert np.array_equal(a["mask_frame_sum"], m.reshape(N, -1).sum(axis=1, dtype=np.int64).astype(np.float64))
    f, y, x = a["sample_frame_row_col"].astype(np.int64).T
    assert len(f) == bench.DUMP_SAMPLE and len(np.unique(f * H * 2 * W + y * 2 * W + x)) == len(f)
    assert np.array_equal(a["sbs_sample"], s[f, y, x].astype(np.float32))
    assert np.array_equal(a["mask_sample"], m[f, y, x].astype(np.float32))
