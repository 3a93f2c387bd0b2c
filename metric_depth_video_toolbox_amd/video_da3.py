"""The host side of the reference's video_da3.py (vd3:), the depth step movie_2_3D.py picks when no engine is named: the command
line, the batch schedule with its reference frames and overlap, the alignment of a batch's camera poses to the batches before, the
file names and the `--generator` loader.  Plain host logic: no tensor's address is taken here.  tools/video_da3.py runs the step on
the device with these pieces (the batch factor from mdvt_scale_shift_fit's sums, the depth video through
step_device.depth_video_codes, the wrapper of mdvt_depth_video_codes).

Two pieces of Depth-Anything-3 that the reference calls cannot be observed without DA3 and are DECREES of this project:
the batch factor (least_squares_scale_scalar: its documented formula, this project's order of summation) and the pose alignment
(align_poses_umeyama: Umeyama's closed form on the camera centres, sim3_from_centres below).  The default `da3` generator is
UNTESTED: DA3 is not available to this project."""
from __future__ import annotations

import argparse
import json

import numpy as np

from .step_clip import add_device_flags, callable_from_spec, clips_from_argument, output_pair, write_float_list  # noqa: F401 (exported)

REFUSED = {                                              # flag -> why the step does not take it: the reference itself cannot run it
    "xfov": "--xfov cannot run in the reference either: video_da3.py:102 reads cam_matrix before it is assigned, and video_da3.py:47-50 "
            "appends the camera matrices to the image list",
    "yfov": "--yfov cannot run in the reference either: video_da3.py:102 reads cam_matrix before it is assigned, and video_da3.py:47-50 "
            "appends the camera matrices to the image list",
    "xfov_file": "--xfov_file cannot run in the reference either: video_da3.py:112 names undefined variables (compute_camera_matrix, "
                 "original_width, original_height), and video_da3.py:47-50 appends the camera matrices to the image list",
    "transformation_file": "--transformation_file cannot run in the reference either: it needs the intrinsics of --xfov / --xfov_file "
                           "(video_da3.py:102, 112, which fail), and video_da3.py:47-50 appends the matrices to the image list",
}


def build_parser():
    p = argparse.ArgumentParser(description="MDVT DepthAnythingV3 video converter")
    p.add_argument("--color_video", type=str, required=True, help="the colour video (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--max_frames", type=int, default=-1, help="maximum length of the input video, -1 means no limit")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses", required=False)
    p.add_argument("--xfov", type=float, help="refused: the reference cannot run it", required=False)
    p.add_argument("--yfov", type=float, help="refused: the reference cannot run it", required=False)
    p.add_argument("--transformation_file", type=str, default=None, help="refused: the reference cannot run it")
    p.add_argument("--xfov_file", type=str, help="refused: the reference cannot run it", required=False)
    p.add_argument("--images_per_batch", default=40, type=int, help="nr of images per batch; set depening on GPU memmory", required=False)
    p.add_argument("--batch_overlap", default=6, type=int, help="nr of images that is overlaped from the last batch", required=False)
    p.add_argument("--nr_of_ref_frames", default=6, type=int, help="nr of references that will be picked spaning the video", required=False)
    p.add_argument("--da3_resolution", default=504, type=int, help="resolution width used in inference. 504 is default 252 good for longer "
                   "videos and GPUs with less ram", required=False)
    p.add_argument("--generator", default="da3", type=str,
                   help="not a reference flag: the depth model, 'da3' (default; needs the depth_anything_3 package) or pkg.module:callable with "
                        "infer(frames, resolution) -> (depth, extrinsics, intrinsics): frames uint8 CUDA [T,H,W,3] RGB, depth float32 CUDA "
                        "[T,h,w], extrinsics [T,3,4] world-to-camera and intrinsics [T,3,3] of any float dtype on either side")
    return add_device_flags(p)


def check_flags(a):
    """NotImplementedError, naming the reason, for the four flags the reference's own code cannot run."""
    for name, why in REFUSED.items():
        if getattr(a, name, None) is not None:
            raise NotImplementedError(why)


def check_schedule_args(images_per_batch, batch_overlap, nr_of_ref_frames):
    if int(images_per_batch) < 1:
        raise ValueError(f"--images_per_batch must be at least 1, got {images_per_batch}")
    if int(batch_overlap) < 0 or int(nr_of_ref_frames) < 0:
        raise ValueError("--batch_overlap and --nr_of_ref_frames must not be negative")


def reference_frame_ids(n: int, nr_of_ref_frames: int):
    """vd3:128-137: every (n // refs)-th frame -- so 100 frames with 6 references give 7 -- or frame 0 alone when n < refs."""
    if nr_of_ref_frames == 0:
        return []
    nth = n // nr_of_ref_frames
    return [0] if nth == 0 else list(range(0, n, nth))


def batch_schedule(n: int, images_per_batch: int, batch_overlap: int, nr_of_ref_frames: int):
    """Per batch (the frames the model sees, how many of them lead as references: nr_used_refs), vd3:140-171 with its quirks.
    The batches are consecutive runs of images_per_batch frames: the model sees references + overlap + that many (the subtraction
    at vd3:141 is never used).  The overlap is batch[-batch_overlap:] of the batch before, so an overlap of 0 hands over the whole
    batch, as Python's slices do."""
    check_schedule_args(images_per_batch, batch_overlap, nr_of_ref_frames)
    refs = reference_frame_ids(int(n), int(nr_of_ref_frames))
    out, last = [], None
    for a in range(0, int(n), int(images_per_batch)):
        batch = list(range(a, min(a + int(images_per_batch), int(n))))
        lead = refs + (last or [])
        out.append((lead + batch, len(lead)))
        last = batch[-int(batch_overlap):]
    return out


# ---- poses: float64 from arrival ------------------------------------------------------------------------------------------------
def pose4(p):
    """[3, 4] (or [4, 4]) -> float64 [4, 4]."""
    p = np.asarray(p, np.float64)
    return np.vstack([p[:3, :4], [0.0, 0.0, 0.0, 1.0]])


def camera_centres(poses):
    """c = -R^T t of world-to-camera poses [n, 3, 4] -> float64 [n, 3]."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    return np.einsum("nji,nj->ni", poses[:, :, :3], -poses[:, :, 3])


IDENTITY_SIM3 = (1.0, np.eye(3), np.zeros(3))


def sim3_from_centres(src, dst):
    """(s, R, t) with dst ~ s R src + t over points [n, 3]: Umeyama's closed form (1991) in float64.  The identity where it is
    undefined -- fewer than 3 points, centres that coincide, values that are not finite -- as the reference goes on unaligned when
    DA3's alignment raises (vd3:207-213)."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    if len(src) < 3 or len(src) != len(dst) or not (np.isfinite(src).all() and np.isfinite(dst).all()):
        return IDENTITY_SIM3
    ms, md = src.mean(0), dst.mean(0)
    xs, xd = src - ms, dst - md
    var = float((xs * xs).sum()) / len(src)
    if not var > 1e-18:
        return IDENTITY_SIM3
    U, D, Vt = np.linalg.svd(xd.T @ xs / len(src))
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    s = float((D * S).sum()) / var
    if not (np.isfinite(s) and s > 0):
        return IDENTITY_SIM3
    R = (U * S) @ Vt
    return s, R, md - s * (R @ ms)


def apply_sim3(poses, s, R, t):
    """The similarity on world-to-camera poses [n, 3, 4]: c' = s R c + t, R' = R_pose R^T, t' = -R' c'."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    out = np.empty_like(poses)
    for k, p in enumerate(poses):
        c = s * (R @ (-p[:, :3].T @ p[:, 3])) + t
        out[k, :, :3] = p[:, :3] @ R.T
        out[k, :, 3] = -out[k, :, :3] @ c
    return out


def last_frame_correction(earlier_last, predicted_last):
    """vd3:219-223: the 4 x 4 `diff` that maps this batch's last reference pose onto the earlier one."""
    return pose4(earlier_last) @ np.linalg.inv(pose4(predicted_last))


def align_batch_poses(earlier, ref_poses, new_poses):
    """vd3:203-228.  earlier: the first batch's reference poses followed by the previous batch's written overlap poses; ref_poses:
    this batch's poses of the same frames; new_poses: its poses of the new frames.  -> the new poses, aligned, float64 [n, 3, 4]."""
    sim = sim3_from_centres(camera_centres(ref_poses), camera_centres(earlier))
    new_poses, ref_poses = apply_sim3(new_poses, *sim), apply_sim3(ref_poses, *sim)
    diff = last_frame_correction(np.asarray(earlier, np.float64)[-1], ref_poses[-1])
    return np.stack([(diff @ pose4(v))[:3] for v in new_poses]) if len(new_poses) else new_poses


class PoseTrack:
    """The poses and intrinsics of a clip as the batches arrive (vd3:198-241, 247-263), all on the host."""

    def __init__(self, batch_overlap: int):
        self.overlap = int(batch_overlap)
        self.first_refs = self.last = None
        self.extrinsics, self.intrinsics = [], []

    def add(self, extrinsics, intrinsics, nr_used_refs: int, scale=None):
        """A batch's [T, 3, 4] and [T, 3, 3] host arrays.  scale: the batch factor (vd3:192 scales every translation), or None."""
        ext = np.array(extrinsics, np.float64).reshape(-1, 3, 4)
        if scale is not None:
            ext[:, :, 3] *= float(scale)
        refs, new = ext[:nr_used_refs], ext[nr_used_refs:]
        if self.first_refs is None:
            self.first_refs = refs.copy()
        if self.last is not None:
            new = align_batch_poses(np.concatenate([self.first_refs, self.last]), refs, new)
        self.extrinsics.extend(new)
        self.intrinsics.extend(np.asarray(intrinsics)[nr_used_refs:])
        self.last = new[-self.overlap:]                              # (an overlap of 0 hands over all of them, as the frames)

    def xfovs(self):
        from .depth_map_tools import fov_from_camera_matrix
        return [float(fov_from_camera_matrix(K)[0]) for K in self.intrinsics]                # vd3:248-251

    def transformations(self):
        return [np.linalg.inv(pose4(e)) for e in self.extrinsics]                            # vd3:256-260: DA3's are the inverse of what the render takes


# ---- files ----------------------------------------------------------------------------------------------------------------------
def output_paths(color_video: str, video: bool = True):
    """(tmp, final, xfovs, transformations): vd3:74-77; a .npy frame dump gives .npy depth frames."""
    tmp, final = output_pair(color_video, video)
    return tmp, final, final + "_xfovs.json", final + "_transformations.json"


def write_json_files(xfov_file: str, transformations_file: str, xfovs, transformations):
    write_float_list(xfov_file, xfovs)
    with open(transformations_file, "w") as fh:
        fh.write(json.dumps([np.asarray(t, np.float64).tolist() for t in transformations]))


# ---- the model ------------------------------------------------------------------------------------------------------------------
class DA3Generator:
    """The default generator: DepthAnything3.inference as vd3:58-63 and 270-276 call it, on host frames.  UNTESTED here (DA3 is not
    available to this project)."""

    def __init__(self, weights: str = "depth-anything/da3nested-giant-large"):
        import importlib
        try:
            api = importlib.import_module("depth_anything_3.api")
        except ImportError as e:
            raise RuntimeError(f"the da3 generator needs the depth_anything_3 package ({e}); install it or name another model with "
                               "--generator pkg.module:callable") from None
        import torch
        self.model = api.DepthAnything3.from_pretrained(weights).to(device=torch.device("cuda"))

    def __call__(self, frames, resolution):
        import torch
        images = list(frames.cpu().numpy())
        p = self.model.inference(images, extrinsics=None, intrinsics=None, process_res=int(resolution))
        depth = torch.as_tensor(np.ascontiguousarray(p.depth, dtype=np.float32)).to(frames.device)
        return depth, np.asarray(p.extrinsics), np.asarray(p.intrinsics)


def load_generator(spec: str):
    """`da3` (the default model) or `pkg.module:callable`."""
    return DA3Generator() if spec == "da3" else callable_from_spec(spec, "da3")

