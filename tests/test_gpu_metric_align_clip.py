"""video_metric_convert end to end on small synthetic dumps: the command line writes `<color_video>_depth.mkv` with the frame count,
holding the codes NumPy gives (tests/metric_align_ref.py), with the host and with the device encoder, from a float32 and from an
RGB-coded reference, and leaves no tmp file behind; and convert() feeding StereoRerenderer.render directly gives the same
side-by-side frames as rendering the file's frames."""
import os

import numpy as np
import pytest

import metric_align_ref as mr

pytestmark = pytest.mark.gpu

F = np.float32
N, w, h, W, H = 6, 40, 22, 64, 36


def _dumps(d, seed=7):
    """-> (colour video path, relative dump path, metric depth [N, h, w], relative [N, h, w], colour frames)"""
    from metric_depth_video_toolbox_amd import video_io
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = np.stack([F(2.0) + F(0.05) * xx + F(0.1) * yy + F(3.0) * ((xx - 8 - 2 * k) ** 2 + (yy - 10) ** 2 < 30) for k in range(N)]).astype(F)
    rel = (F(1) / depth * F(1.7) + F(0.05) + rng.normal(0, 0.002, depth.shape).astype(F)).astype(F)
    color = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    cp = str(d / "x.mkv")
    with video_io.VideoWriter(cp, W, H, 24000 / 1001) as wr:
        for f in color:
            wr.write(f)
    np.save(d / "rel.npy", rel)
    return cp, str(d / "rel.npy"), depth, rel, color


def _read(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        assert (r.width, r.height) == (W, H)
        frames = np.empty((r.frames, H, W, 3), np.uint8)
        for k in range(r.frames):
            assert r.read_into(frames[k])
        return frames, r.fps


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_cli_writes_numpys_codes(tmp_path, encoder):
    from metric_depth_video_toolbox_amd import video_io, video_metric_convert as vmc
    cp, rp, depth, rel, _ = _dumps(tmp_path)
    np.save(tmp_path / "ref.npy", depth)
    for engine, style in (("vda", 0), ("depthcrafter", 1)):
        assert vmc.main(["--color_video", cp, "--relative_depth", rp, "--metric_depth", str(tmp_path / "ref.npy"), "--engine", engine,
                         "--batch", "4", "--video_encoder", encoder]) == 0
        f = mr.fit(mr.concat(rel), mr.concat(mr.inverse(depth)))
        want = mr.metric_codes(rel, f[5], f[6], 100, style, (W, H))[0]
        got, fps = _read(cp + "_depth.mkv")
        assert got.shape[0] == N and abs(fps - 24000 / 1001) < 1e-3
        assert np.array_equal(got, want), engine
        os.remove(cp + "_depth.mkv")
    # an RGB-coded reference video, decoded by the existing decode; max_depth 20, 5 frames
    ref_codes = mr.code(depth, 20)[1]
    with video_io.VideoWriter(str(tmp_path / "ref.mkv"), w, h, 24.0) as wr:
        for fr in ref_codes:
            wr.write(np.ascontiguousarray(fr))
    assert vmc.main(["--color_video", cp, "--relative_depth", rp, "--depth_video", str(tmp_path / "ref.mkv"), "--max_depth", "20", "--max_frames", "5",
                     "--video_encoder", encoder, "--video_decoder", encoder]) == 0
    u = (ref_codes[..., 0].astype(np.uint32) << 24) | (ref_codes[..., 2].astype(np.uint32) << 16)
    seen = u.astype(F) * F(20 / 255 ** 4)                           # dfh:21-23
    f = mr.fit(mr.concat(rel[:5]), mr.concat(mr.inverse(seen[:5])))
    got, _ = _read(cp + "_depth.mkv")
    assert got.shape[0] == 5 and np.array_equal(got, mr.metric_codes(rel[:5], f[5], f[6], 20, 0, (W, H))[0])
    assert sorted(os.listdir(tmp_path)) == ["ref.mkv", "ref.npy", "rel.npy", "x.mkv", "x.mkv_depth.mkv"]      # no tmp file is left


def test_a_failure_in_the_batch_loop_leaves_no_file(tmp_path, monkeypatch):
    """The second batch fails: the sink is closed, the tmp file is removed, no output file appears, the error comes through."""
    from metric_depth_video_toolbox_amd import video_metric_convert as vmc
    cp, rp, depth, rel, _ = _dumps(tmp_path)
    np.save(tmp_path / "ref.npy", depth)
    real, calls = vmc.metric_depth_codes, []

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("second batch")
        return real(*a, **kw)
    monkeypatch.setattr(vmc, "metric_depth_codes", failing)
    with pytest.raises(RuntimeError, match="second batch"):
        vmc.run(cp, rp, metric_depth=str(tmp_path / "ref.npy"), batch=4)
    assert len(calls) == 2
    assert sorted(os.listdir(tmp_path)) == ["ref.npy", "rel.npy", "x.mkv"]


def test_convert_feeds_the_renderer_like_the_file_does(tmp_path):
    import torch
    from metric_depth_video_toolbox_amd import video_metric_convert as vmc
    from metric_depth_video_toolbox_amd.stereo_rerender import StereoRerenderer
    cp, rp, depth, rel, color = _dumps(tmp_path, seed=9)
    np.save(tmp_path / "ref.npy", depth)
    vmc.run(cp, rp, metric_depth=str(tmp_path / "ref.npy"))
    filed, _ = _read(cp + "_depth.mkv")
    codes = vmc.convert(torch.from_numpy(rel).cuda(), torch.from_numpy(depth).cuda(), 100, out_size=(W, H))
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (N, H, W, 3)
    r = StereoRerenderer(W, H, device=0, pupillary_distance=65)
    try:
        p = r.frame_params(xfov=50.0)
        for k in range(N):
            c = torch.from_numpy(color[k]).cuda()
            direct = r.render(codes[k], c, p)["sbs"].cpu().numpy()
            via_file = r.render(torch.from_numpy(filed[k]).cuda(), c, p)["sbs"].cpu().numpy()
            assert np.array_equal(direct, via_file), k
        assert direct.shape == (H, 2 * W, 3) and direct.any()
    finally:
        r.close()
