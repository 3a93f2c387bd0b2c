"""NumPy restatement of the free-camera viewer's centre (include/mdvt_view.h): the vertices of oracle_np.unproject (the chain of
orc_unproject_f64), Open3D's point transform as tests/golden/gen_golden.py:_O3dPoints restates it, the parking of dmt:1091 and
np.sum over each coordinate's contiguous array.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import c_oracle as co
from oracle import oracle_np as onp

PARKED = -0.2                                            # dmt:1091


def o3d_transform(P, T):
    """Geometry3D::TransformPoints in f64: the 4 x 4 times (x, y, z, 1), sums left to right, divided by its w."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    h = [((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3] * 1.0 for r in range(4)]
    return np.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], axis=1)


def vertices(depth_rgb, K, *, mesh, remove_edges=False, T=None, max_depth=100.0, depth_scale=1.0):
    """The vertices draw_mesh holds at 3dv:231 for one frame: [H W, 3] f64."""
    depth = onp.decode_rgb_depth_frame(depth_rgb, max_depth, depth_scale)
    P = onp.unproject(depth, K, of_by_one=mesh)
    if T is not None:
        P = o3d_transform(P, T)
    if remove_edges and not mesh:
        _tri, unused, _n = co.edge_filter(depth, K, of_by_one=False)
        P = P.copy()
        P[unused != 0] = PARKED
    return P


def center_of(P):
    """S_c / N with S_c = np.sum of the contiguous f64 array of coordinate c."""
    return np.array([np.sum(np.ascontiguousarray(P[:, c])) / np.float64(P.shape[0]) for c in range(3)], np.float64)


def center(depth_rgb, K, **kw):
    return center_of(vertices(depth_rgb, K, **kw))


def center_bound(P):
    """What two orders of summation may differ by, per coordinate: 2 (N - 1) 2^-53 sum |v| / N (include/mdvt_view.h)."""
    n = P.shape[0]
    return 2.0 * (n - 1) * 2.0 ** -53 * np.abs(P).sum(axis=0) / n
