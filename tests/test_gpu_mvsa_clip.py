"""tools/video_mvsa.py end to end on a 64 x 36 colour clip of 12 frames with a stub in the model's place: the depth video byte for byte
and the cost-volume scales equal to the NumPy restatement of the whole step (tests/mvsa_ref.run_step), the host and the device
codecs giving the same file, a list file, --max_frames, --window 7 and 1, a one-frame clip, --transformation_file in the list and the
dict form, --apply_cost_volume_scale on and off, no tmp file left.

The stub is a deterministic function of the planes it is handed (so a frame that reached the model changed, or a wrong reference
frame, shows up in the file): the refined depth is one multiply and one add on the target's red plane, the cost volume's depth, at
half resolution, one multiply and one add on the first reference's green plane, the mask a threshold on the last reference's blue
plane.  It asserts the two dicts' keys, shapes and devices, and that the reference frames are those of reference_indices."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

import metric_align_ref as mr
import mvsa_ref as vr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N, W, H = 12, 64, 36
RESIZE_W, MW, MH = 96, 96, 54                                       # 96 + 54 > 128: the two-pass form of the bilinear resize
MAX_DEPTH, BATCH = 20, 3                                           # a ring of 10 frames under --window 7: it wraps, and a batch is split at its end
CUR_KEYS = {"image_b3hw", "K_s0_b44", "invK_s0_b44", "K_matching_b44", "invK_matching_b44", "K_full_depth_b44", "invK_full_depth_b44",
            "cam_T_world_b44", "world_T_cam_b44", "frame_id_string", "full_res_depth_b1hw"}


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("video_mvsa_tool", os.path.join(REPO, "tools", "video_mvsa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stub(image, refs, i, ref_idx, mask=True):
    """float32 [3, h, w], [R, 3, h, w] -> (depth [h, w], lowest cost [h / 2, w / 2], mask uint8 [h / 2, w / 2] or None)."""
    assert image.dtype == np.float32 and image.shape == (3, MH, MW) and refs.shape == (len(ref_idx), 3, MH, MW)
    depth = (image[0] * F(24) + F(0.5)).astype(F)                   # up to 24.5: beyond max_depth
    cv = (refs[0, 1, ::2, ::2] * F(30) + F(0.25)).astype(F)
    cv[::5, ::7] = F(-1)                                            # pixels without a cost-volume depth
    return depth, cv, (refs[-1, 2, ::2, ::2] > F(0.3)).astype(np.uint8) if mask else None


class OnDevice:
    """The stub under the generator's contract: dicts of CUDA tensors in, a dict of CUDA tensors out; it checks what it is handed."""

    def __init__(self, n, window, mask_key="overall_mask_bhw", transforms=None, fast=False):
        self.n, self.window, self.mask_key, self.transforms, self.fast, self.calls = n, window, mask_key, transforms, fast, 0

    def __call__(self, cur, src, fast_cost_volume):
        import torch
        from metric_depth_video_toolbox_amd import video_mvsa as host
        i = self.calls
        self.calls += 1
        ref_idx = host.reference_indices(i, self.n, self.window)
        R = len(ref_idx)
        assert fast_cost_volume is self.fast
        assert set(cur) == CUR_KEYS and set(src) == CUR_KEYS - {"full_res_depth_b1hw"}
        assert cur["frame_id_string"] == [f"{i:06d}"] and src["frame_id_string"] == [f"{j:06d}" for j in ref_idx]
        assert cur["image_b3hw"].shape == (1, 3, MH, MW) and src["image_b3hw"].shape == (1, R, 3, MH, MW)
        assert cur["full_res_depth_b1hw"].shape == (1, 1, H, W) and not cur["full_res_depth_b1hw"].any()
        for k in CUR_KEYS - {"image_b3hw", "frame_id_string", "full_res_depth_b1hw"}:
            assert cur[k].shape == (1, 4, 4) and src[k].shape == (1, R, 4, 4), k
        for d in (cur, src):
            assert all(t.is_cuda and t.dtype == torch.float32 for t in d.values() if isinstance(t, torch.Tensor))
        K = cur["K_full_depth_b44"][0].cpu()
        assert torch.equal(cur["K_s0_b44"][0].cpu(), torch.diag(torch.tensor([1.5, 1.5, 1, 1])) @ K) and torch.equal(cur["K_s0_b44"], cur["K_matching_b44"])
        assert torch.equal(cur["invK_s0_b44"][0].cpu(), torch.inverse(cur["K_s0_b44"][0].cpu())) and float(K[0, 2]) == W / 2
        assert torch.equal(src["K_s0_b44"][0], cur["K_s0_b44"].expand(R, 4, 4)) and torch.equal(src["invK_full_depth_b44"][0, -1], cur["invK_full_depth_b44"][0])
        T = np.tile(np.eye(4, dtype=F), (self.n, 1, 1)) if self.transforms is None else self.transforms
        assert np.array_equal(cur["cam_T_world_b44"][0].cpu().numpy(), T[i]) and np.array_equal(src["cam_T_world_b44"][0].cpu().numpy(), T[ref_idx])
        assert torch.equal(cur["world_T_cam_b44"][0].cpu(), torch.inverse(torch.from_numpy(T[i])))
        assert np.allclose(src["world_T_cam_b44"][0].cpu().numpy(), np.linalg.inv(T[ref_idx].astype(np.float64)), rtol=1e-5, atol=1e-6)
        depth, cv, mask = stub(cur["image_b3hw"][0].cpu().numpy(), src["image_b3hw"][0].cpu().numpy(), i, ref_idx, self.mask_key is not None)
        dev = cur["image_b3hw"].device
        out = {"depth_pred_s0_b1hw": torch.from_numpy(depth)[None, None].to(dev), "lowest_cost_bhw": torch.from_numpy(cv)[None].to(dev)}
        if self.mask_key == "overall_mask_bhw":
            out[self.mask_key] = torch.from_numpy(mask)[None].to(dev).to(torch.bool)
        elif self.mask_key == "overall_mask_b1hw":
            out[self.mask_key] = torch.from_numpy(mask)[None, None].to(dev).float()
        return out


# ---- the clips ----------------------------------------------------------------------------------------------------------------------
def _write(path, frames, fps=24.0):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoWriter(path, frames.shape[2], frames.shape[1], fps) as wr:
        for f in frames:
            wr.write(f)
    return path


def _read(path):
    from metric_depth_video_toolbox_amd import video_io
    with video_io.VideoReader(path) as r:
        frames = np.empty((r.frames, r.height, r.width, 3), np.uint8)
        for k in range(r.frames):
            assert r.read_into(frames[k])
        return frames


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("mvsa")
    color = np.random.default_rng(11).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    return d, _write(str(d / "x.mkv"), color), color


def _args(path, *more):
    from metric_depth_video_toolbox_amd import video_mvsa
    return video_mvsa.build_parser().parse_args(["--color_video", path, "--xfov", "60", "--max_depth", str(MAX_DEPTH), "--batch", str(BATCH),
                                                 "--resize_w", str(RESIZE_W)] + list(more))


def _restated(color, window, apply_scale=False, mask=True):
    return vr.run_step(color, lambda *a: stub(*a, mask=mask), resize_w=RESIZE_W, window=window, max_depth=MAX_DEPTH, apply_scale=apply_scale)


@pytest.fixture(scope="module")
def host_route(tool, clip):
    """--window 7 with the scales saved, on the host codecs, and the restatement: computed once, shared."""
    d, path, color = clip
    os.mkdir(d / "host")
    mine = shutil.copy(path, str(d / "host" / "x.mkv"))
    model = OnDevice(N, 7)
    written = tool.run(_args(mine, "--save_cost_volume_scales"), model)
    return mine, written, model, _restated(color, 7)


def test_the_depth_video_and_the_scales_equal_the_restatement(host_route):
    mine, written, model, (codes, scales) = host_route
    assert written == [mine + "_depth.mkv"] and model.calls == N
    assert sorted(os.listdir(os.path.dirname(mine))) == ["x.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_cv_scales.json"]      # no tmp file is left
    got = _read(mine + "_depth.mkv")
    assert got.shape == (N, H, W, 3) and np.array_equal(got, codes)
    saved = json.load(open(mine + "_depth.mkv_cv_scales.json"))
    assert saved == [float(s) for s in scales] and len(set(saved)) == N and all(np.isfinite(saved)) and 1.0 not in saved
    top = (got == mr.code(np.full((1, 1), MAX_DEPTH, F), MAX_DEPTH)[1][0, 0]).all(-1)     # the code of max_depth itself
    assert 0 < top.mean() < 0.5, "some depths lie beyond max_depth and take the clip"


@pytest.mark.parametrize("decoder", ["device", "device_all"])
def test_the_device_codecs_give_the_host_routes_file(tool, host_route, tmp_path, decoder):
    mine = host_route[0]
    other = shutil.copy(mine, str(tmp_path / "x.mkv"))
    tool.run(_args(other, "--video_decoder", decoder, "--video_encoder", "device", "--save_cost_volume_scales"), OnDevice(N, 7))
    assert sorted(os.listdir(tmp_path)) == ["x.mkv", "x.mkv_depth.mkv", "x.mkv_depth.mkv_cv_scales.json"]
    for tail in ("_depth.mkv", "_depth.mkv_cv_scales.json"):
        assert open(other + tail, "rb").read() == open(mine + tail, "rb").read(), tail


def test_applying_the_scale_multiplies_each_frame_by_its_median(tool, clip, host_route, tmp_path):
    _, path, color = clip
    other = shutil.copy(path, str(tmp_path / "x.mkv"))
    tool.run(_args(other, "--apply_cost_volume_scale"), OnDevice(N, 7))
    assert sorted(os.listdir(tmp_path)) == ["x.mkv", "x.mkv_depth.mkv"]                # the scales are written on request only
    codes, scales = _restated(color, 7, apply_scale=True)
    got = _read(other + "_depth.mkv")
    assert np.array_equal(got, codes) and not np.array_equal(got, host_route[3][0]) and np.array_equal(scales, host_route[3][1])


def test_a_list_file_max_frames_window_1_and_the_other_mask_key(tool, clip, tmp_path):
    _, path, color = clip
    a, b = shutil.copy(path, str(tmp_path / "a.mkv")), shutil.copy(path, str(tmp_path / "b.mkv"))
    lst = tmp_path / "list.txt"
    lst.write_text(f"# two clips\n{a}\n\n{b}\n")

    class Twice:
        def __init__(self):
            self.models, self.calls = [OnDevice(7, 1, "overall_mask_b1hw", fast=True), OnDevice(7, 1, "overall_mask_b1hw", fast=True)], 0

        def __call__(self, *args):
            self.calls += 1
            return self.models[(self.calls - 1) // 7](*args)
    model = Twice()
    written = tool.run(_args(str(lst), "--max_frames", "7", "--window", "1", "--fast_cost_volume", "--save_cost_volume_scales"), model)
    assert written == [a + "_depth.mkv", b + "_depth.mkv"] and model.calls == 14
    codes, scales = _restated(color[:7], 1)
    for out in written:
        got = _read(out)
        assert got.shape[0] == 7 and np.array_equal(got, codes)
        assert json.load(open(out + "_cv_scales.json")) == [float(s) for s in scales]


def test_a_clip_of_one_frame_refers_to_itself_and_no_mask_key_means_no_mask(tool, clip, tmp_path):
    _, _, color = clip
    one = _write(str(tmp_path / "one.mkv"), color[3:4])
    tool.run(_args(one, "--save_cost_volume_scales", "--apply_cost_volume_scale"), OnDevice(1, 7, None))
    codes, scales = _restated(color[3:4], 7, apply_scale=True, mask=False)
    assert np.array_equal(_read(one + "_depth.mkv"), codes) and json.load(open(one + "_depth.mkv_cv_scales.json")) == [float(scales[0])]
    masked = _restated(color[3:4], 7, mask=True)[1]
    assert masked[0] != scales[0], "the stub's mask changes the median: without the key none was applied"


@pytest.mark.parametrize("form", ["list", "dict"])
def test_the_transformation_file_reaches_the_model_in_both_forms(tool, clip, tmp_path, form):
    _, path, color = clip
    rng = np.random.default_rng(12)
    T = np.tile(np.eye(4), (N, 1, 1))
    for k in range(N):
        a = 0.02 * k
        T[k, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        T[k, :3, 3] = rng.normal(size=3)
    if form == "list":
        data = [T[k].tolist() if k % 2 else {"cam_T_world": T[k].reshape(-1).tolist()} for k in range(N)]
    else:
        data = {str(k): (T[k].tolist() if k % 2 else {"cam_T_world": T[k].tolist()}) for k in range(N) if k != 5}
        T[5] = np.eye(4)                                            # a frame the file does not name keeps the identity
    tf = tmp_path / "t.json"
    tf.write_text(json.dumps(data))
    other = shutil.copy(path, str(tmp_path / "x.mkv"))
    model = OnDevice(N, 8, transforms=T.astype(F))
    tool.run(_args(other, "--transformation_file", str(tf), "--window", "8"), model)
    assert model.calls == N and np.array_equal(_read(other + "_depth.mkv"), _restated(color, 8)[0])
