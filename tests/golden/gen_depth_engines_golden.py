"""Writes tests/golden/depth_engines.npz: inputs and outputs of the reference's estimate_focal_lengths (unik3d_video.py:22-101, on torch
CPU) and of fov_from_camera_matrix as unik3d_video.py, moge_video.py and depthpro_video.py each call it, run on the build machine only:

    python tests/golden/gen_depth_engines_golden.py /path/to/the/reference/checkout

The scripts are imported under stub modules (their models, cv2 and the viewer's packages are absent; only functions that never touch
them are called).  Inputs come from seeded generators; nothing of the reference is stored but results.

  focal_<case>_points    float32 point maps, [B, H, W, 3] or [B, 3, H, W] with B = 1, as handed to the function
  focal_<case>_ex, _ey   float32 [H, W]: est_fx, est_fy as the function's torch.where leaves them (0 where not selected), captured from
                         the function itself: its module's `torch` is wrapped for the duration of the call
  focal_<case>_mx, _my   bool [H, W]: valid_mask_x, valid_mask_y, captured likewise
  focal_<case>_f         float32 [2]: the returned fx, fy (torch CPU's mean)
  fov_unik3d_in          float64 [n, 4]: fx, fy (float32 values), width, height;   fov_unik3d_out  float64 [n]: float(fovx), u3d:176-183
  fov_moge_in            float32 [n, 3, 3] intrinsics;                             fov_moge_out    float64 [n]: float(fovx), mge:165-167
  fov_depthpro_in        float64 [n, 3]: focallength_px (a float32 value), width, height;  fov_depthpro_out  float64 [n], dpr:152-159
  chm_in, chm_out        int64: closest_higher_multiple(x) (upscale_depth_promptda.py:16-17)
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(ref):
    for name in ("cv2", "glfw", "OpenGL", "OpenGL.GL", "open3d", "unik3d", "unik3d.utils", "moge", "depth_pro", "promptda"):
        _stub(name)
    _stub("OpenGL.GL.shaders", compileProgram=None, compileShader=None)
    _stub("unik3d.models", UniK3D=None)
    _stub("unik3d.utils.camera", Pinhole=None)
    _stub("moge.model", MoGeModel=None)
    _stub("promptda.promptda", PromptDA=None)
    sys.path.insert(0, ref)
    import depth_map_tools as dmt
    import depthpro_video as dpr
    import moge_video as mge
    import unik3d_video as u3d
    import upscale_depth_promptda as pda
    return dmt, u3d, mge, dpr, pda


class _TorchTap:
    """torch, except that where() remembers its condition and its result."""

    def __init__(self, torch):
        self._torch, self.seen = torch, []

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def where(self, cond, a, b):
        out = self._torch.where(cond, a, b)
        self.seen.append((cond.clone(), out.clone()))
        return out


def run_focal(u3d, points):
    import torch
    tap = _TorchTap(torch)
    u3d.torch = tap
    try:
        t = torch.from_numpy(points)
        H, W = (t.shape[1], t.shape[2]) if t.shape[-1] == 3 else (t.shape[2], t.shape[3])
        fx, fy = u3d.estimate_focal_lengths(t, W, H)
    finally:
        u3d.torch = torch
    (mx, ex), (my, ey) = tap.seen
    assert ex.dtype == torch.float32 and mx.dtype == torch.bool and ex.shape == (1, H, W)
    return dict(ex=ex[0].numpy(), ey=ey[0].numpy(), mx=mx[0].numpy(), my=my[0].numpy(), f=np.array([float(fx), float(fy)], F))


def pinhole_points(rng, H, W, fx, fy, noise):
    """A point map of a pinhole camera with its principal point in the middle, depth in [0.5, 20], and multiplicative noise on X and Y."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    Z = rng.uniform(0.5, 20.0, (H, W))
    X = (u - W / 2.0) * Z / fx * (1.0 + rng.normal(0, noise, (H, W)))
    Y = (v - H / 2.0) * Z / fy * (1.0 + rng.normal(0, noise, (H, W)))
    return np.stack([X, Y, Z], axis=-1).astype(F)


def special_values():
    eps = F(1e-6)
    return [eps, np.nextafter(eps, F(1)), np.nextafter(eps, F(0)), -eps, -np.nextafter(eps, F(1)), -np.nextafter(eps, F(0)),
            F(0.0), F(-0.0), F(np.nan), F(np.inf), F(-np.inf), F(1e-30), F(3e38), F(-2.5)]


def focal_cases():
    rng = np.random.default_rng(20263)
    p = pinhole_points(rng, 96, 96, 83.25, 79.5, 0.02)
    drop = rng.random((96, 96))
    p[drop < 0.08, 0] = 0.0                                              # nx != ny
    p[(drop > 0.90) & (drop < 0.93), 1] = 1e-7
    p[drop > 0.97, 2] = np.nan
    yield "noisy96", np.ascontiguousarray(p.transpose(2, 0, 1))[None]    # [1, 3, H, W]
    yield "clean40x30", pinhole_points(rng, 30, 40, 31.0, 33.5, 0.0)[None]      # [1, H, W, 3]
    sp = special_values()
    p = pinhole_points(rng, 3, 7, 5.0, 4.0, 0.1)
    for k in range(21):                                                  # every special value meets X, Y and Z somewhere
        p[k // 7, k % 7, k % 3] = sp[k % len(sp)]
    p[1, 2] = (sp[1], sp[2], sp[1])
    p[2, 5] = (np.inf, 1.0, np.inf)
    yield "special7x3", p[None]
    p = pinhole_points(rng, 3, 7, 5.0, 4.0, 0.1)
    p[..., 2] = 0.0                                                      # selects nothing: 0.0
    yield "empty7x3", p[None]


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    import torch
    dmt, u3d, mge, dpr, pda = import_reference(argv[1])
    out = {}
    for name, points in focal_cases():
        got = run_focal(u3d, points)
        out[f"focal_{name}_points"] = points
        for k, v in got.items():
            out[f"focal_{name}_{k}"] = v
        print(name, points.shape, "fx, fy =", got["f"], "selected", int(got["mx"].sum()), int(got["my"].sum()))
    rng = np.random.default_rng(20264)
    sizes = [(1920, 1080), (64, 36), (960, 540), (13, 7), (3840, 2160)]
    # unik3d: a torch float32 scalar stored into the float64 matrix (u3d:176-183)
    rows, fov = [], []
    for k in range(12):
        W, H = sizes[k % len(sizes)]
        fx, fy = (F(0.0), F(0.0)) if k == 11 else (F(rng.uniform(0.2, 3.0) * W), F(rng.uniform(0.2, 3.0) * W))
        cam = dmt.compute_camera_matrix(90, None, W, H)
        cam[0][0] = torch.tensor(fx)
        cam[1][1] = torch.tensor(fy)
        rows.append([float(fx), float(fy), W, H])
        fov.append(float(dmt.fov_from_camera_matrix(cam)[0]))
    out["fov_unik3d_in"], out["fov_unik3d_out"] = np.array(rows, np.float64), np.array(fov, np.float64)
    # moge: the model's float32 intrinsics (mge:165-167)
    Ks, fov = [], []
    for k in range(12):
        K = np.eye(3, dtype=F)
        K[0, 0], K[1, 1] = F(rng.uniform(0.3, 3.0)), F(rng.uniform(0.3, 3.0))
        K[0, 2], K[1, 2] = (F(0.5), F(0.5)) if k % 2 == 0 else (F(rng.uniform(0.4, 0.6)), F(rng.uniform(0.4, 0.6)))
        Ks.append(K)
        fov.append(float(mge.fov_from_camera_matrix(torch.from_numpy(K).cpu().numpy())[0]))
    out["fov_moge_in"], out["fov_moge_out"] = np.stack(Ks), np.array(fov, np.float64)
    # depthpro: float(focallength_px) twice (dpr:152-159)
    rows, fov = [], []
    for k in range(12):
        W, H = sizes[k % len(sizes)]
        f = torch.tensor(F(rng.uniform(0.2, 3.0) * W))
        cam = dpr.compute_camera_matrix(90, None, W, H)
        cam[0][0] = float(f)
        cam[1][1] = float(f)
        rows.append([float(f), W, H])
        fov.append(float(dpr.fov_from_camera_matrix(cam)[0]))
    out["fov_depthpro_in"], out["fov_depthpro_out"] = np.array(rows, np.float64), np.array(fov, np.float64)
    xs = np.array([1, 13, 14, 15, 27, 28, 29, 36, 64, 540, 1078, 1080, 1092, 1920, 2160, 3840], np.int64)
    out["chm_in"], out["chm_out"] = xs, np.array([pda.closest_higher_multiple(int(x)) for x in xs], np.int64)
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "torch": torch.__version__}))
    path = os.path.join(HERE, "depth_engines.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), f"{path}: {size} bytes"
    print(f"{path}: {size} bytes")


if __name__ == "__main__":
    main(sys.argv)
