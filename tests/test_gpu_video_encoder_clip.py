"""--video_encoder device end to end: every .mkv output of the CLI is byte-identical to the host encoder's run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(d, W, H, N, config_id=3):
    from metric_depth_video_toolbox_amd import video_io
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene
    dep, col = SyntheticScene(W, H, config_id=config_id, n_fg=5).clip(N)
    dp, cp = str(d / "v_depth.mkv"), str(d / "v.mkv")
    for path, frames in ((dp, dep), (cp, col)):
        with video_io.VideoWriter(path, W, H, 24000 / 1001, bgr=True) as w:
            for f in frames:
                w.write(np.ascontiguousarray(f[..., ::-1]))
    return dp, cp


def _outputs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("v_depth.mkv_")}


@pytest.mark.parametrize("variant", ["product_default", "points"])
def test_device_encoder_writes_the_host_bytes(tmp_path, variant, monkeypatch):
    from metric_depth_video_toolbox_amd import ffv1_device, stereo_rerender as sr
    collected = []
    collect = ffv1_device.PendingPackets.collect

    def counting_collect(self, *a, **k):          # every device-mode batch, and whether the host had to step in
        out = collect(self, *a, **k)
        collected.append((len(out), self.host_frames))
        return out
    monkeypatch.setattr(ffv1_device.PendingPackets, "collect", counting_collect)
    W, H, N = 160, 90, 11
    flags = ["--xfov", "50", "--pupillary_distance", "65", "--create_sbs_depth_video", "--batch", "4"]
    if variant == "points":
        flags += ["--render_as_pointcloud"]
    else:
        (tmp_path / "conv.json").write_text(json.dumps([2.5 + 0.02 * k if k % 5 else float("nan") for k in range(N)]))
        flags += ["--infill_mask", "--convergence_file", str(tmp_path / "conv.json")]
    outs = {}
    for enc in ("host", "device"):
        d = tmp_path / enc
        d.mkdir()
        dp, cp = _inputs(d, W, H, N)
        assert sr.main(["--depth_video", dp, "--color_video", cp, "--video_encoder", enc] + flags) == 0
        outs[enc] = _outputs(d)
    want = {"v_depth.mkv_stereo.mkv", "v_depth.mkv_stereo.mkv_holemask.mkv", "v_depth.mkv_stereo.mkv_depth.mkv"}
    if variant == "product_default":
        want.add("v_depth.mkv_stereo.mkv_infillmask.mkv")
    # the device run encoded every frame of every output itself
    assert sum(n for n, _ in collected) == len(want) * N and all(h == 0 for _, h in collected)
    assert set(outs["host"]) == want and set(outs["device"]) == want
    for f in want:
        assert outs["device"][f] == outs["host"][f], f


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_on_one_gpu_write_the_host_bytes(tmp_path):
    W, H, N = 256, 144, 13
    outs = {}
    for enc in ("host", "device"):
        d = tmp_path / enc
        d.mkdir()
        dp, cp = _inputs(d, W, H, N)
        env = dict(os.environ, MDVT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=REPO)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), "-m", "metric_depth_video_toolbox_amd.stereo_rerender",
               "--depth_video", dp, "--color_video", cp, "--xfov", "45", "--pupillary_distance", "65", "--batch", "4",
               "--infill_mask", "--create_sbs_depth_video", "--video_encoder", enc]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert p.returncode == 0 and "Processing complete" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        outs[enc] = _outputs(d)
    assert outs["host"] and set(outs["host"]) == set(outs["device"])
    assert any("rank1of2" in f for f in outs["host"])
    for f in outs["host"]:
        assert outs["device"][f] == outs["host"][f], f
