"""The host side of the reference's sam_track_video.py (stv:), the depth-assisted camera-tracking step around MegaSAM's DROID tracker:
the command line, the file names, the tracker's image size, the scaled intrinsics, which frames the reference's look-ahead loop hands
over, the poses' way into a transformation file and the `--generator` loader.  Plain host logic in NumPy: torch is not imported here
and no tensor's address is taken.  tools/sam_track_video.py runs the step on the device with these pieces and
megasam_device.py's wrappers of the four entry points of include/mdvt_megasam.h.

DECREES of this project: the pose conversion is the closed form in float64, because lietorch's
SE3(...).inv().matrix() cannot be observed; the JSON holds t + 1 matrices, the identity first (stv:240); frame_plan reproduces the
reference's one-frame look-ahead loop, quirks included; the estimated field of view is printed from intrinsics[0] * 8 (stv:210-245).
The default `megasam` tracker is UNTESTED: neither droid nor lietorch is available to this project."""
from __future__ import annotations

import argparse
import json

import numpy as np

from .depth_map_tools import compute_camera_matrix, fov_from_camera_matrix
from .step_clip import add_device_flags, callable_from_spec

MEGASAM_DROID_PATH = "mega-sam/base/droid_slam"                       # stv:12
MEGASAM_WEIGHTS_PATH = "mega-sam/checkpoints/megasam_final.pth"       # stv:172


def build_parser():
    """stv:27-35 under its names, and the flags that are not the reference's."""
    p = argparse.ArgumentParser(description="Mega-sam camera tracker")
    p.add_argument("--color_video", type=str, required=True)
    p.add_argument("--depth_video", type=str, help="depth video", required=True)
    p.add_argument("--mask_video", type=str, help="black and white mask video for thigns that should not be tracked", required=False)
    p.add_argument("--max_frames", type=int, default=-1, help="maximum length of the input video, -1 means no limit")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses", required=False)
    p.add_argument("--xfov", type=float, help="fov in deg in the x-direction, calculated from aspectratio and yfov in not given", required=False)
    p.add_argument("--yfov", type=float, help="fov in deg in the y-direction, calculated from aspectratio and xfov in not given", required=False)
    p.add_argument("--optimize_intrinsic", action="store_true", help="Optimize camera instrinsics (ie FOV)", required=False)
    p.add_argument("--generator", default="megasam", type=str,
                   help="not a reference flag: the tracker, 'megasam' (default; needs droid and lietorch) or pkg.module:callable with "
                        "make_tracker(image_size) -> tracker (INTEGRATION.md states the contract)")
    return add_device_flags(p, 8, "frames per read and per resize call")


def check_flags(a):
    """What is refused before any file is opened, each with its reason."""
    if a.xfov is None and a.yfov is None:
        raise ValueError("Either --xfov or --yfov is required.")       # stv:39-41 prints this and exits
    if int(a.batch) < 1:
        raise ValueError(f"--batch must be at least 1, got {a.batch}")
    if not (int(a.max_depth) > 0):
        raise ValueError(f"--max_depth must be > 0, got {a.max_depth}")


def output_paths(depth_video: str, video: bool = True):
    """stv:46, 233-234 -> {"json", "depth", "motion"}: (tmp, final) each; the tmp names are this project's.  A .npy frame dump
    gives .npy frames."""
    ext = ".mkv" if video else ".npy"
    return {"json": (depth_video + "_tmp_transformations.json", depth_video + "_transformations.json"),
            "depth": (depth_video + "_tmp_megasam" + ext, depth_video + "_megasam" + ext),
            "motion": (depth_video + "_tmp_megasam_motion" + ext, depth_video + "_megasam_motion" + ext)}


def model_size(h0: int, w0: int):
    """stv:134-144 -> (h1, w1, hc, wc): the resized size in NumPy float64, and its crop to multiples of 8."""
    h1 = int(h0 * np.sqrt((384 * 512) / (h0 * w0)))
    w1 = int(w0 * np.sqrt((384 * 512) / (h0 * w0)))
    return h1, w1, h1 - h1 % 8, w1 - w1 % 8


def camera_matrix(xfov, yfov, width: int, height: int):
    """stv:68: float32 [3, 3]."""
    return compute_camera_matrix(xfov, yfov, width, height).astype(np.float32)


def scaled_intrinsics(cam_matrix, h0: int, w0: int, h1: int, w1: int):
    """stv:138-140 -> float32 [4] = (fx, fy, cx, cy) at the tracker's size: a float32 tensor times a Python float, which torch
    multiplies in float32 with the factor rounded to float32 first."""
    k = np.array([cam_matrix[0][0], cam_matrix[1][1], cam_matrix[0][2], cam_matrix[1][2]], dtype=np.float32)
    k[0::2] *= np.float32(w1 / w0)
    k[1::2] *= np.float32(h1 / h0)
    return k


def frame_plan(n_depth: int, n_color: int, n_mask, max_frames: int):
    """Which frames stv:78-198 hands to the tracker -> (count, final_index): frames 0 .. count - 1 go over, and frame final_index
    (None: none) goes through track_final instead of track.  The reference's loop buffers one frame to know the last one, and is
    followed read by read, quirks included: with equal lengths the last frame is never handed over, because the colour read behind
    it ends the loop; --max_frames M hands over M + 2 frames.  A colour or mask video shorter than the depth video is a ValueError:
    the reference crashes there, on the missing frame."""
    n = {"depth": int(n_depth), "color": int(n_color), "mask": None if n_mask is None else int(n_mask)}
    max_frames = int(max_frames)
    for name in ("color", "mask"):
        if n[name] is not None and n[name] < n["depth"]:
            raise ValueError(f"the {name} video has {n[name]} frames, the depth video {n['depth']}: sam_track_video.py crashes on the "
                             "missing frame")
    pos = {"depth": 0, "color": 0, "mask": 0}

    def read(name):                                                 # cv2.VideoCapture.read's `ret`
        ok = pos[name] < n[name]
        pos[name] += ok
        return ok

    masked = n["mask"] is not None
    have_next, fr_n, final, final_index = False, 0, False, None
    while True:
        if not have_next:                                           # stv:81-91
            if not read("depth") or not read("color") or (masked and not read("mask")):
                break
        have_next = read("depth")                                   # stv:101-105
        if not have_next and final:
            break
        if not have_next:
            final = True
        if not read("color") and final:                             # stv:107-109
            break
        if masked and not read("mask") and final:                   # stv:111-114
            break
        if max_frames < fr_n and max_frames != -1:                  # stv:119-122
            if final:
                break
            final = True
        if final:                                                   # stv:193-196
            final_index = fr_n
        fr_n += 1
    return fr_n, final_index


def poses_to_transformations(traj):
    """stv:236-240 -> float64 [t + 1, 4, 4]: the inverse of every pose as a 4 x 4 matrix, behind an identity.  traj: [t, 7] as
    tx ty tz qx qy qz qw, the quaternion of unit length (lietorch's SE3 data).  DECREE: the closed form in float64 -- R from the
    quaternion, the inverse [R^T | -R^T t] -- where the reference calls lietorch's SE3(...).inv().matrix(), which cannot be observed."""
    traj = np.asarray(traj, dtype=np.float64)
    if traj.ndim != 2 or traj.shape[1] != 7:
        raise ValueError(f"the tracker's trajectory must be [t, 7] (tx ty tz qx qy qz qw), got shape {traj.shape}")
    out = np.zeros((traj.shape[0] + 1, 4, 4), dtype=np.float64)
    out[:, 3, 3] = 1.0
    out[0, :3, :3] = np.eye(3)
    for i, (tx, ty, tz, x, y, z, w) in enumerate(traj, start=1):
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)
        out[i, :3, :3] = R.T
        out[i, :3, 3] = -(R.T @ np.array([tx, ty, tz], dtype=np.float64))
    return out


def write_transformations(tmp: str, final: str, transformations):
    """stv:239-241, under a temporary name first."""
    import os
    with open(tmp, "w") as fh:
        fh.write(json.dumps(np.asarray(transformations).tolist()))
    os.replace(tmp, final)


def estimated_fov(intrinsics0):
    """stv:210-217, 244: (fovx, fovy) in degrees from the first frame's estimated (fx, fy, cx, cy) at an eighth of the tracker's size."""
    k = np.asarray(intrinsics0, dtype=np.float32) * 8
    est = np.eye(3)
    est[0, 0], est[1, 1], est[0, 2], est[1, 2] = k[0], k[1], k[2], k[3]
    return fov_from_camera_matrix(est)


DROID_ARGS = {"disable_vis": True, "stereo": False, "upsample": False, "buffer": 1024, "beta": 0.3, "filter_thresh": 2.0, "warmup": 8,   # stv:170-188
              "keyframe_thresh": 2.0, "frontend_thresh": 12.0, "frontend_window": 25, "frontend_radius": 2, "frontend_nms": 1,
              "backend_thresh": 16.0, "backend_radius": 2, "backend_nms": 3}


class MegaSamTracker:
    """stv:169-206 around droid.Droid.  UNTESTED here (neither droid nor lietorch is available to this project)."""

    def __init__(self, image_size, weights: str = MEGASAM_WEIGHTS_PATH, droid_path: str = MEGASAM_DROID_PATH):
        import importlib
        import sys
        from types import SimpleNamespace
        sys.path.append(droid_path)
        try:
            droid = importlib.import_module("droid")
            importlib.import_module("lietorch")
        except ImportError as e:
            raise RuntimeError(f"the megasam tracker needs droid and lietorch ({e}); install them or name another tracker with "
                               "--generator pkg.module:callable") from None
        self.droid = droid.Droid(SimpleNamespace(image_size=[int(image_size[0]), int(image_size[1])], weights=weights, **DROID_ARGS))

    def track(self, t, image, depth, intrinsics, mask):
        self.droid.track(t, image, depth, intrinsics, mask)

    def track_final(self, t, image, depth, intrinsics, mask):
        self.droid.track_final(t, image, depth, intrinsics, mask)

    def terminate(self, stream, optimize_intrinsic):
        traj, depth, motion = self.droid.terminate(iter(stream), _opt_intr=bool(optimize_intrinsic), full_ba=True, scene_name="output_scene")
        intr = self.droid.video.intrinsics                          # stv:210; the results go back onto its device
        on_device = lambda v: intr.new_tensor(np.asarray(v, dtype=np.float32)).float()          # noqa: E731
        return on_device(traj), on_device(depth), on_device(motion), intr[:len(traj)].float()


def load_generator(spec: str):
    """`megasam` (the default tracker) or `pkg.module:callable`: make_tracker(image_size) -> tracker."""
    return MegaSamTracker if spec == "megasam" else callable_from_spec(spec, "megasam")
