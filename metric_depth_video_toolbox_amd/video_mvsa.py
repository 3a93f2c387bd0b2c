"""The host side of the reference's video_mvsa.py (mvs:), the MVSAnywhere depth step that takes camera poses on the way in: the command
line, the three forms of a transformation file, the window of reference frames with its quirks, the model's size, the intrinsics and
their inverses exactly as the script computes them, the file names and the `--generator` loader.  Plain host logic: no tensor's
address is taken here.  tools/video_mvsa.py runs the step on the device with these pieces and step_device.py's wrappers of the three
entry points of include/mdvt_mvsa.h.

Three DECREES of this project: the frames go into the model through the unfused float32 bilinear formula, because torch's
CPU bilinear has no single set of bits; the two nearest resizes and the median are held to torch's CPU kernels, because CUDA's cannot
be observed; and --apply_cost_volume_scale, off by default, is this project's reading of the `* s` the reference comments out
(mvs:297), not the reference's output.  The default `mvsanywhere` generator is UNTESTED: MVSAnywhere is not available to this project."""
from __future__ import annotations

import argparse
import json

import numpy as np

from .depth_map_tools import compute_camera_matrix
from .step_clip import add_device_flags, callable_from_spec, clips_from_argument, output_pair, write_float_list  # noqa: F401 (exported)

MVSA_CONFIG_PATH = "mvsanywhere/configs/models/mvsanywhere_model.yaml"          # mvs:16-17
MVSA_WEIGHTS_PATH = "mvsanywhere/weights/mvsanywhere_hero.ckpt"


def build_parser():
    """mvs:67-79 under its names, and the flags that are not the reference's."""
    p = argparse.ArgumentParser(description="Convert a video together with camera poses into metric depth video using MVSAnywhere")
    p.add_argument("--color_video", required=True, type=str, help="the colour video (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--xfov", type=float, required=False)
    p.add_argument("--yfov", type=float, required=False)
    p.add_argument("--transformation_file", type=str, default=None)
    p.add_argument("--max_frames", type=int, default=-1)
    p.add_argument("--window", type=int, default=7, help="ref count around target (odd recommended)")
    p.add_argument("--resize_w", type=int, default=1024, help="model input width; keeps aspect")
    p.add_argument("--fast_cost_volume", action="store_true")
    p.add_argument("--max_depth", type=int, default=100)
    p.add_argument("--apply_cost_volume_scale", action="store_true",
                   help="not a reference flag: multiply each frame's depth by the median ratio the reference computes and leaves unused "
                        "(video_mvsa.py:283-297); this project's reading of the author's intent, not the reference's output")
    p.add_argument("--save_cost_volume_scales", action="store_true",
                   help="not a reference flag: write the per-frame median ratios to x.mkv_depth.mkv_cv_scales.json")
    p.add_argument("--generator", default="mvsanywhere", type=str,
                   help="not a reference flag: the model, 'mvsanywhere' (default; needs the mvsanywhere package) or pkg.module:callable with "
                        "infer(cur_data, src_data, fast_cost_volume) -> dict of CUDA tensors (INTEGRATION.md states the contract)")
    return add_device_flags(p, 8, "frames per read and per resize call")


def check_flags(a):
    """What is refused before any file is opened, each with its reason."""
    if a.xfov is None and a.yfov is None:
        raise ValueError("--xfov or --yfov is required: video_mvsa.py:102 computes the camera matrix from them, and with neither "
                         "compute_camera_matrix has no focal length")
    if int(a.batch) < 1:
        raise ValueError(f"--batch must be at least 1, got {a.batch}")
    if int(a.resize_w) < 1:
        raise ValueError(f"--resize_w must be at least 1, got {a.resize_w}")


def frames_to_read(n_in_file: int, max_frames: int) -> int:
    """mvs:90-96: all frames, or the first max_frames where max_frames > 0 (0 and negatives mean no limit)."""
    n = int(n_in_file)
    return min(n, int(max_frames)) if int(max_frames) > 0 else n


# ---- poses ----------------------------------------------------------------------------------------------------------------------
def _to44(x, where):
    """mvs:29-34: 16 values in any shape, or a 4 x 4; where the reference's assert fails this is a ValueError naming the entry."""
    try:
        arr = np.array(x, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"transformation {where} is not a 4x4 matrix of numbers") from None
    if arr.size == 16:
        arr = arr.reshape(4, 4)
    if arr.shape != (4, 4):
        raise ValueError(f"transformation {where} is not 4x4: shape {arr.shape}")
    return arr


def transforms_from_data(data, n_frames: int):
    """mvs:23, 36-56 on parsed JSON -> float32 [N, 4, 4] cam_T_world, the identity wherever the data names nothing.
    A list: entry i is frame i's -- a dict with "cam_T_world" or "Tcw" (other dicts are skipped), or the matrix itself.
    A dict: key "i" is frame i's -- a dict with "cam_T_world", or the matrix itself; keys that are no integer or no frame are skipped."""
    T = np.stack([np.eye(4, dtype=np.float32) for _ in range(int(n_frames))]) if n_frames else np.zeros((0, 4, 4), np.float32)
    if isinstance(data, list):
        for i, elem in enumerate(data[:n_frames]):
            if isinstance(elem, dict):
                if "cam_T_world" in elem:
                    T[i] = _to44(elem["cam_T_world"], i)
                elif "Tcw" in elem:
                    T[i] = _to44(elem["Tcw"], i)
            elif isinstance(elem, (list, tuple, np.ndarray)):
                T[i] = _to44(elem, i)
    elif isinstance(data, dict):
        for k, v in data.items():
            try:
                idx = int(k)
            except (TypeError, ValueError):
                continue
            if 0 <= idx < n_frames:
                T[idx] = _to44(v["cam_T_world"] if isinstance(v, dict) and "cam_T_world" in v else v, repr(k))
    return T


def load_transforms(json_path, n_frames: int):
    """mvs:21-56 -> float32 [N, 4, 4]; the identity without a file."""
    if not json_path:
        return transforms_from_data(None, n_frames)
    with open(json_path, "r") as f:
        return transforms_from_data(json.load(f), n_frames)


def check_transformation_file(json_path):
    """The ValueError of a transformation that is not 4x4, for every entry of the file whatever the clip's length, before any output is
    opened (the reference's assert at mvs:33 fails after the model has been loaded)."""
    if not json_path:
        return
    with open(json_path, "r") as f:
        data = json.load(f)
    if isinstance(data, list):
        transforms_from_data(data, len(data))
    elif isinstance(data, dict):
        ids = [int(k) for k in data if str(k).lstrip("-").isdigit()]
        transforms_from_data(data, max(ids) + 1 if ids else 0)


# ---- the window, the sizes, the intrinsics ----------------------------------------------------------------------------------------
def half_window(window: int) -> int:
    """mvs:146: an even window behaves as the next odd one, and --window 1 (or 0) still takes one neighbour on each side."""
    return max(1, int(window) // 2)


def reference_indices(i: int, n: int, window: int):
    """mvs:152-161: the frames i - half .. i + half inside the clip without i; where that is empty (a one-frame clip) the single index
    min(n - 1, max(0, i + 1)), so the frame refers to itself."""
    half = half_window(window)
    ref = [j for j in range(i - half, i + half + 1) if 0 <= j < n and j != i]
    return ref if ref else [min(n - 1, max(0, i + 1))]


def model_size(width: int, height: int, resize_w: int):
    """mvs:136-138 -> (newW, newH, scale): Python's round (halves to even) on float64 products."""
    scale = resize_w / float(width)
    return int(round(width * scale)), int(round(height * scale)), scale


def intrinsics(xfov, yfov, width: int, height: int, resize_w: int):
    """mvs:102-107, 136-144 -> (K44, invK44, K44_s, invK44_s), CPU float32 tensors [4, 4], by exactly the reference's calls."""
    import torch
    cam = compute_camera_matrix(xfov, yfov, width, height)
    K44 = torch.eye(4, dtype=torch.float32)
    K44[:3, :3] = torch.from_numpy(cam).float()
    invK44 = torch.inverse(K44)
    scale = model_size(width, height, resize_w)[2]
    S = torch.tensor([[scale, 0, 0, 0], [0, scale, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    K44_s = S @ K44
    return K44, invK44, K44_s, torch.inverse(K44_s)


# ---- files ----------------------------------------------------------------------------------------------------------------------
def output_paths(color_video: str, video: bool = True):
    """(tmp, final, scales): mvs:303 names the final file; tmp and the scales' file are this project's.  A .npy frame dump gives .npy
    depth frames."""
    tmp, final = output_pair(color_video, video)
    return tmp, final, final + "_cv_scales.json"


write_scales = write_float_list


# ---- the model ------------------------------------------------------------------------------------------------------------------
class MVSAnywhereGenerator:
    """mvs:113-132, 234-242.  UNTESTED here (MVSAnywhere is not available to this project)."""

    def __init__(self, config: str = MVSA_CONFIG_PATH, weights: str = MVSA_WEIGHTS_PATH):
        import importlib
        try:
            utils = importlib.import_module("mvsanywhere.utils.model_utils")
        except ImportError as e:
            raise RuntimeError(f"the mvsanywhere generator needs the mvsanywhere package ({e}); install it or name another model with "
                               "--generator pkg.module:callable") from None
        from types import SimpleNamespace
        opts = SimpleNamespace(model_type="depth_model", config_file=config, load_weights_from_checkpoint=weights, precision=16,
                               fast_cost_volume=False, name="mvsa_video_infer", prediction_scale=1.0, prediction_num_scales=1)
        self.model = utils.load_model_inference(opts, utils.get_model_class(opts)).cuda().eval()

    def __call__(self, cur_data, src_data, fast_cost_volume):
        import torch
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            return self.model(phase="test", cur_data=cur_data, src_data=src_data,
                              unbatched_matching_encoder_forward=(not fast_cost_volume), return_mask=True, num_refinement_steps=1)


def load_generator(spec: str):
    """`mvsanywhere` (the default model) or `pkg.module:callable`."""
    return MVSAnywhereGenerator() if spec == "mvsanywhere" else callable_from_spec(spec, "mvsanywhere")
