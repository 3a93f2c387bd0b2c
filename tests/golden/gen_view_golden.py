#!/usr/bin/env python3
"""Generate tests/golden/view_look_at.npz by importing the reference's own pure-NumPy functions (the stub-import recipe of
gen_golden.py): what pins the camera side of metric_depth_video_toolbox_amd/view_depthfile.py.

Run ONLY in the build container (needs the reference tree).  Nothing of the reference travels: the fixture holds inputs and the
reference functions' outputs.

    python tests/golden/gen_view_golden.py

  look_pos [n, 3] f32, look_target [n, 3] f64, look_mat [n, 4, 4] f64      dmt.cam_look_at(cam_pos, target) (dmt:1618-1638), the
                                                                           3dv:239 camera positions (float32) among them
  depth_rgb [H, W, 3] u8, K [3, 3] f64, max_depth                          one depth frame and its camera matrix (3dv:98, 164)
  vertices_mesh / vertices_points [H W, 3] f64                             dmt.create_point_cloud_from_depth(depth, K, of_by_one)
  mean_mesh / mean_points [3] f64                                          their .mean(axis=0): NumPy adds the rows one after the
                                                                           other, as Open3D's get_center adds the vertices
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from gen_golden import import_reference  # noqa: E402


def main():
    dfh, dmt, _sr, _ic = import_reference()
    from metric_depth_video_toolbox_amd.synthetic import SyntheticScene

    pos = np.array([[2.0, 2.0, -4.0], [0.0, 0.0, 0.0], [-1.5, 0.25, 3.0], [0.1, -7.3, 0.2], [1e-3, 2.5, -1e3], [2.0, 2.0, -4.0]]).astype(np.float32)
    target = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, 1.0], [0.3337, -0.21, 7.75], [4.0, 1.0, -2.0], [12.5, -0.125, 40.0],
                       [-0.01690625, 0.0371, 2.9140625]], np.float64)
    mats = np.stack([dmt.cam_look_at(p.copy(), t.copy()) for p, t in zip(pos, target)])

    W, H, max_depth = 64, 48, 100
    depth_rgb, _color = SyntheticScene(W, H, config_id=1, n_fg=4).frame(0)
    depth_rgb = np.ascontiguousarray(depth_rgb)
    depth_rgb[5, 7] = 0                                                      # a depth code 0
    K = dmt.compute_camera_matrix(60, None, W, H)
    depth = dfh.decode_rgb_depth_frame(depth_rgb, max_depth, True)
    out = dict(look_pos=pos, look_target=target, look_mat=mats, depth_rgb=depth_rgb, K=np.asarray(K, np.float64),
               max_depth=np.float64(max_depth))
    for name, of_by_one in (("mesh", True), ("points", False)):
        pts, h, w = dmt.create_point_cloud_from_depth(depth, K, of_by_one)
        assert (h, w) == (H, W) and pts.dtype == np.float64 and pts.shape == (H * W, 3)
        out["vertices_" + name] = pts
        out["mean_" + name] = pts.mean(axis=0)
    out["meta"] = np.array(json.dumps({"numpy": np.__version__}))
    np.savez_compressed(os.path.join(HERE, "view_look_at.npz"), **out)
    print("wrote view_look_at.npz", os.path.getsize(os.path.join(HERE, "view_look_at.npz")), "bytes")


if __name__ == "__main__":
    main()
