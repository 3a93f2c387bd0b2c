"""bench.py --dump-outputs on the hardware: the files hold what the timed path computed -- the same bytes as a render of the
bench's own synthetic frames in this process -- and the line reports exactly the --steps it was given."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dumped_outputs_are_the_timed_path_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from metric_depth_video_toolbox_amd.stereo_rerender import StereoRerenderer
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    W, H, N = 256, 144, 4
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "1",
                        "--frames", str(N), "--width", str(W), "--height", str(H), "--no-extra", "--no-cpu-baseline",
                        "--prewarm-ms", "0", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 7 and line["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["mask.npy", "sbs.npy"]
    sbs, mask = np.load(tmp_path / "sbs.npy"), np.load(tmp_path / "mask.npy")
    assert sbs.dtype == np.float32 and sbs.shape == (N, H, 2 * W, 3) and mask.dtype == np.float32 and mask.shape == (N, H, 2 * W)

    d, c = SyntheticScene(W, H, config_id=2).clip(N, t0=0)
    r = StereoRerenderer(W, H, device=0, pupillary_distance=65, max_depth=100.0, master_xfov=45.0, render_as_pointcloud=True,
                         remove_edges=False, dont_place_points_in_edges=True)
    got = r.render(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), [r.frame_params(xfov=45.0) for _ in range(N)])
    torch.cuda.synchronize()
    assert np.array_equal(sbs, got["sbs"].cpu().numpy().astype(np.float32))
    assert np.array_equal(mask, got["mask"].cpu().numpy().astype(np.float32))
    assert (mask > 0).any()
    r.close()


def test_plain_line_is_the_headline_only():
    """Without --full the run ends after the timed steps: the line has the headline and its roofline, no extras and no CPU
    baseline (what --full adds is checked by tests/test_gpu_distributed.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames", "4", "--width", "256", "--height", "144", "--prewarm-ms", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "stereo frames/s" and line["higher_is_better"] is True and line["roofline"]["bound"] == "hbm"
    assert line["extra"] == {} and line["cpu_baseline"] is None
