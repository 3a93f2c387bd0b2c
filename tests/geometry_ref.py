"""NumPy and oracle restatement of the geometry export (include/mdvt_geometry.h): the depth of the two decodes in NumPy, the vertices
and the filter's flags from oracle.c_oracle (unproject_f64, edge_filter), the lists from the flags with np.flatnonzero and the
topology of dmt:1243-1254, the pose as tests/view_ref.py restates Open3D's, and the grey depth of cmf:752-760.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import c_oracle as co

import view_ref

CODE_MAX = 255 ** 4                                      # the encoder's own maximum (dfh:13-24)


def codes(depth_rgb, decode):
    """The uint32 code of every pixel: R << 24 | B << 16 (decode 1, dfh:67-69) or ((R + G) >> 1) << 24 | B << 16 (decode 0, cmf:648-649)."""
    rgb = np.asarray(depth_rgb, np.uint8)
    r, g, b = (rgb[..., k].astype(np.uint32) for k in range(3))
    hi = r if decode else (r + g) >> 1
    return (hi << 24) | (b << 16)


def depth_of(depth_rgb, decode, max_depth, depth_scale=1.0):
    """f32 depth of a frame.  decode 1: f32(code) * f32(max_depth / 255^4); decode 0: f32(code) / f32(255^4 / max_depth), one
    correctly rounded division; both * f32(depth_scale)."""
    c = codes(depth_rgb, decode).astype(np.float32)
    if decode:
        d = c * np.float32(max_depth / CODE_MAX)
    else:
        d = c / np.float32(CODE_MAX / max_depth)
    return d * np.float32(depth_scale)


def topology(W, H):
    """triangles_all of dmt:1243-1254: [2 (H-1) (W-1), 3] int32."""
    gi, gj = np.meshgrid(np.arange(H - 1), np.arange(W - 1), indexing="ij")
    gi, gj = gi.ravel(), gj.ravel()
    i1, i2, i3, i4 = gi * W + gj, (gi + 1) * W + gj, (gi + 1) * W + gj + 1, gi * W + gj + 1
    return np.vstack([np.stack([i1, i2, i3], 1), np.stack([i1, i3, i4], 1)]).astype(np.int32)


def lists_from_flags(tri_invalid, W, H):
    """(kept triangles [M, 3] int32 in draw order, used vertices [U] int32 ascending) from the filter's flags (dmt:1378-1384)."""
    tris = topology(W, H)[np.flatnonzero(np.asarray(tri_invalid) == 0)]
    used = np.zeros(W * H, bool)
    used[tris.ravel()] = True
    return tris, np.flatnonzero(used).astype(np.int32)


class Frame:
    """Everything the export gives for one frame: vertices [N, 3] f64 (posed), triangles [M, 3] i32, used_index [U] i32,
    points [U, 3] f64, point_rgb [U, 3] u8 (None without a colour frame), counts (U, M)."""


def export(depth_rgb, K, *, decode, remove_edges, max_depth=100.0, depth_scale=1.0, T=None, color_rgb=None):
    H, W = depth_rgb.shape[:2]
    depth = depth_of(depth_rgb, decode, max_depth, depth_scale)
    P = co.unproject_f64(depth, K, True)
    if remove_edges:
        tri_invalid, _unused, _n = co.edge_filter(depth, K, True)
    else:
        tri_invalid = np.zeros(2 * (H - 1) * (W - 1), np.uint8)
    f = Frame()
    f.depth, f.unposed, f.tri_invalid = depth, P, tri_invalid
    f.triangles, f.used_index = lists_from_flags(tri_invalid, W, H)
    f.vertices = view_ref.o3d_transform(P, T) if T is not None else P
    f.points = f.vertices[f.used_index]
    f.point_rgb = None if color_rgb is None else np.asarray(color_rgb, np.uint8).reshape(-1, 3)[f.used_index]
    f.counts = (len(f.used_index), len(f.triangles))
    return f


def grey(depth_rgb, max_depth, bits):
    """(values as NumPy computes them in f32 before the cast, in_range mask, saturated result).  bits 16: u16 [H, W]; 8: u8 [H, W, 3]."""
    d = depth_of(depth_rgb, 0, max_depth)
    top = 65535 if bits == 16 else 255
    v = np.rint(d * np.float32((255 ** 2 if bits == 16 else 255) / max_depth))
    ok = v <= top
    out = np.minimum(v, np.float32(top)).astype(np.uint16 if bits == 16 else np.uint8)
    if bits == 8:
        out = np.repeat(out[..., np.newaxis], 3, axis=-1)
    return v, ok, out
