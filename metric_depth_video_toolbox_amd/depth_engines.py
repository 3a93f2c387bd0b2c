"""The host side of the reference's per-frame depth engines -- unik3d_video.py (u3d:), moge_video.py (mge:), depthpro_video.py (dpr:)
-- and of its PromptDA upscaler, upscale_depth_promptda.py (pda:): the command lines, the file names, the `--generator` loader and the
x-fov arithmetic exactly as each script does it on the host.  Plain host logic: no tensor's address is taken here.
tools/depth_engine_video.py and tools/upscale_depth_promptda.py run the steps on the device with these pieces and step_device.py's
wrappers of the three entry points of include/mdvt_depth_engines.h.

The x-fov of all three engines is fov_from_camera_matrix (dmt:1640; mge:21-30 and dpr:51-60 carry copies of it); what differs is the
matrix it is given:
  unik3d    a float64 camera matrix (compute_camera_matrix(90, None, W, H)) with the float32 fx, fy of the focal estimate stored
            into it (u3d:176-181): float64 arithmetic on float32 values
  moge      the model's float32 intrinsics as they are (mge:165-166): float32 arithmetic throughout
  depthpro  the same float64 matrix with float(focallength_px) as both focal lengths (dpr:152-157)

Two scripts of the family are refused (REFUSED_SCRIPTS).  The default wrappers of the models are UNTESTED: unik3d, moge, depth_pro
and promptda are not available to this project."""
from __future__ import annotations

import argparse
import math

import numpy as np

from . import video_da3
from .depth_map_tools import compute_camera_matrix, fov_from_camera_matrix
from .step_clip import add_device_flags, clips_from_argument, frames_to_write, output_pair, write_float_list  # noqa: F401 (exported)

ENGINES = ("unik3d", "moge", "depthpro")
PROMPT_W, PROMPT_H = 256, 192                            # pda:37: rescale_height, rescale_width = 192, 256

REFUSED_SCRIPTS = {
    "unidepth": "unidepth_video.py cannot run in the reference either: its last line (unidepth_video.py:80) hands save_depth_video an "
                "undefined `fps`, so the script fails with a NameError after the last frame and writes no depth video",
    "videoanythingmetric": "videoanythingmetric_video.py reads its frames with the model repository's own reader "
                           "(utils.dc_utils.read_video_frames, videoanythingmetric_video.py:13, 37, 43), which resizes and resamples them "
                           "inside Video-Depth-Anything: the frames the model sees are not this project's to produce",
}


def check_engine(engine: str):
    """The engine's name, or the NotImplementedError of a script that is left out, naming the reason."""
    if engine in REFUSED_SCRIPTS:
        raise NotImplementedError(REFUSED_SCRIPTS[engine])
    if engine not in ENGINES:
        raise ValueError(f"--engine must be one of {', '.join(ENGINES)}, got {engine!r}")
    return engine


BATCH_HELP = "frames per read, per call of the model and per read-back"


def build_engine_parser():
    """The flags of u3d:114-120, mge:106-112 and dpr:100-104 under their names, and the ones that are not the reference's."""
    p = argparse.ArgumentParser(description="MDVT per-frame metric depth video converter (UniK3D, MoGe, DepthPro)")
    p.add_argument("--engine", type=str, required=True,
                   help="not a reference flag: which script's step to run -- " + ", ".join(ENGINES) + " (unidepth and videoanythingmetric are refused)")
    p.add_argument("--color_video", type=str, required=True, help="the colour video (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--max_frames", type=int, default=-1, help="maximum length of the input video, -1 means no limit")
    p.add_argument("--target_fps", type=int, default=-1, help="target fps of the input video, -1 means the original fps (unused, as in the reference)")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses", required=False)
    p.add_argument("--xfov", type=float, help="fov in deg in the x-direction, calculated from aspectratio and yfov in not given", required=False)
    p.add_argument("--yfov", type=float, help="fov in deg in the y-direction, calculated from aspectratio and xfov in not given", required=False)
    p.add_argument("--generator", default=None, type=str,
                   help="not a reference flag: the model, by default the engine's own (needs its package), or pkg.module:callable with "
                        "infer(frames, camera_or_fov) -> dict of CUDA tensors (INTEGRATION.md states the contract)")
    return add_device_flags(p, 8, BATCH_HELP)


def build_promptda_parser():
    """pda:20-24 under its names, and the flags that are not the reference's."""
    p = argparse.ArgumentParser(description="PromptDA depth video upscaling")
    p.add_argument("--color_video", type=str, required=True)
    p.add_argument("--depth_video", type=str, required=True)
    p.add_argument("--max_frames", type=int, default=-1, help="maximum length of the input video, -1 means no limit")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses", required=False)
    p.add_argument("--generator", default="promptda", type=str,
                   help="not a reference flag: the model, 'promptda' (default; needs the promptda package) or pkg.module:callable with "
                        "upscale(rgb, prompt) -> depth: rgb float32 CUDA [n,3,h14,w14], prompt float32 CUDA [n,1,192,256], depth float32 CUDA [n,h14,w14]")
    return add_device_flags(p, 4, BATCH_HELP)


def check_engine_flags(a):
    """What is refused before any file is opened: a left-out script, and --xfov / --yfov where the script has no such flag."""
    check_engine(a.engine)
    if a.engine == "depthpro" and (a.xfov is not None or a.yfov is not None):
        raise ValueError("depthpro_video.py takes no --xfov / --yfov (dpr:100-104)")
    if int(a.batch) < 1:
        raise ValueError(f"--batch must be at least 1, got {a.batch}")


# ---- files ----------------------------------------------------------------------------------------------------------------------
def engine_output_paths(color_video: str, video: bool = True):
    """(tmp, final, xfovs): u3d:149-151.  moge and depthpro write the final name at once (mge:141, dpr:129); this project writes every
    depth video as tmp and renames it when its frame count is right.  A .npy frame dump gives .npy depth frames."""
    return video_da3.output_paths(color_video, video)[:3]


def promptda_output_paths(depth_video: str, video: bool = True):
    """(tmp, final): pda:84 names the final file; tmp is this project's."""
    return output_pair(depth_video, video, "upscaled")


write_xfovs = write_float_list


def closest_higher_multiple(x, base=14):
    """pda:16-17."""
    return math.ceil(x / base) * base


# ---- the x-fov, per script --------------------------------------------------------------------------------------------------------
def requested_camera(xfov, yfov, width: int, height: int):
    """u3d:143, mge:135: the float32 camera matrix of --xfov / --yfov, or None where neither is given."""
    if xfov is None and yfov is None:
        return None
    return compute_camera_matrix(xfov, yfov, width, height).astype(np.float32)


def xfov_unik3d(fx, fy, width: int, height: int) -> float:
    """u3d:176-183: the focal estimate's float32 fx, fy stored into a float64 matrix."""
    cam = compute_camera_matrix(90, None, width, height)
    cam[0][0] = np.float32(fx)
    cam[1][1] = np.float32(fy)
    return float(fov_from_camera_matrix(cam)[0])


def xfov_moge(intrinsics) -> float:
    """mge:165-167 on float32 intrinsics [3, 3]: every step of fov_from_camera_matrix in float32 (what NumPy gives a float32 scalar
    and a Python int), spelled out so that it does not depend on NumPy's promotion rules."""
    F = np.float32
    K = np.asarray(intrinsics, F)
    w = F(K[0][2] * F(2))
    return float(np.rad2deg(F(F(2) * np.arctan2(w, F(F(2) * K[0][0])))))


def xfov_depthpro(focallength_px, width: int, height: int) -> float:
    """dpr:152-159: float(focallength_px) as both focal lengths of a float64 matrix."""
    cam = compute_camera_matrix(90, None, width, height)
    cam[0][0] = cam[1][1] = float(focallength_px)
    return float(fov_from_camera_matrix(cam)[0])


# ---- the models -------------------------------------------------------------------------------------------------------------------
def _need(package: str, engine: str):
    import importlib
    try:
        return importlib.import_module(package)
    except ImportError as e:
        raise RuntimeError(f"the {engine} generator needs the {package.split('.')[0]} package ({e}); install it or name another model "
                           "with --generator pkg.module:callable") from None


class UniK3DGenerator:
    """u3d:103-112, 168-171 per frame of a batch.  UNTESTED here."""

    def __init__(self):
        models, self.camera = _need("unik3d.models", "unik3d"), _need("unik3d.utils.camera", "unik3d")
        import torch
        model = models.UniK3D.from_pretrained("lpiccinelli/unik3d-vitl")
        model.resolution_level = 9
        model.interpolation_mode = "bilinear"
        self.model = model.to(torch.device("cuda")).eval()

    def __call__(self, frames, cam_matrix):
        import torch
        depth, points = [], []
        for frame in frames:                                            # uint8 [3, H, W]
            camera = None
            if cam_matrix is not None:                                   # a new camera per frame: unik3d modifies the instance (u3d:169)
                camera = self.camera.Pinhole(params=torch.tensor([cam_matrix[0][0], cam_matrix[1][1], cam_matrix[0][2], cam_matrix[1][2]]).float())
            p = self.model.infer(frame, camera)
            depth.append(p["depth"].squeeze().float())
            points.append(p["points"].reshape(3, *frame.shape[1:]).float())
        return {"depth": torch.stack(depth), "points": torch.stack(points)}


class MoGeGenerator:
    """mge:138, 162 per frame of a batch.  UNTESTED here."""

    def __init__(self):
        model = _need("moge.model", "moge")
        import torch
        self.model = model.MoGeModel.from_pretrained("Ruicheng/moge-vitl").to(torch.device("cuda")).eval()

    def __call__(self, frames, fov_x):
        import torch
        out = [self.model.infer(frame, fov_x=fov_x) for frame in frames]         # float32 [3, H, W] in [0, 1]
        return {"depth": torch.stack([o["depth"] for o in out]), "intrinsics": torch.stack([o["intrinsics"] for o in out])}


class DepthProGenerator:
    """dpr:123-124, 144-147 per frame of a batch; DepthPro's own transform stays in here.  UNTESTED here."""

    def __init__(self):
        depth_pro = _need("depth_pro", "depthpro")
        import torch
        model, self.transform = depth_pro.create_model_and_transforms()
        self.model = model.to(torch.device("cuda")).eval()

    def __call__(self, frames, _unused):
        import torch
        out = [self.model.infer(self.transform(frame.permute(1, 2, 0).cpu().numpy()).to(frame.device), f_px=None) for frame in frames]
        return {"depth": torch.stack([o["depth"] for o in out]),
                "focallength_px": torch.stack([torch.as_tensor(o["focallength_px"]).reshape(()) for o in out])}


class PromptDAGenerator:
    """pda:36, 73.  UNTESTED here."""

    def __init__(self):
        promptda = _need("promptda.promptda", "promptda")
        import torch
        self.model = promptda.PromptDA.from_pretrained("depth-anything/prompt-depth-anything-vitl").to(torch.device("cuda")).eval()

    def __call__(self, rgb, prompt):
        import torch
        return torch.stack([self.model.predict(rgb[k:k + 1], prompt[k:k + 1]).squeeze().detach() for k in range(rgb.shape[0])])


_DEFAULTS = {"unik3d": UniK3DGenerator, "moge": MoGeGenerator, "depthpro": DepthProGenerator, "promptda": PromptDAGenerator}


def load_generator(spec, default_name: str):
    """The default model of `default_name` (spec None or that name) or `pkg.module:callable`, through video_da3.load_generator."""
    if spec is None or spec == default_name:
        return _DEFAULTS[default_name]()
    if spec == "da3":
        raise ValueError(f"--generator must be '{default_name}' or 'pkg.module:callable', got {spec!r}")
    return video_da3.load_generator(spec)
