"""Point-cloud and mesh files of the geometry export (include/mdvt_geometry.h; tools/export_depth_geometry.py): .ply and .obj from
host arrays.  NumPy only: importable without torch and without the library.

    write_ply(path, points, colors_u8)              what cmf:743-749 hands o3d.io.write_point_cloud
    write_obj(path, vertices, colors_u8, triangles) what cmf:732-742 hands o3d.io.write_triangle_mesh
    read_ply(path) -> (points f64 [U, 3], colors u8 [U, 3])
    read_obj(path) -> (vertices f64 [N, 3], colors u8 [N, 3], triangles i32 [M, 3], 0-based)

DECREE.  The reference writes these files with Open3D, whose exact bytes cannot be observed here (there is no Open3D): the layouts
below are this project's own, chosen to be what Open3D's writers produce in kind -- a binary little-endian PLY with double
coordinates and uchar colours, an OBJ with `v x y z r g b` and 1-based `f a b c` -- and to lose nothing:
  PLY  header `ply / format binary_little_endian 1.0 / comment Created by Open3D / element vertex U / property double x, y, z /
       property uchar red, green, blue / end_header`, then U records of 27 bytes.  The colour byte is the input byte: the reference's
       byte / 255.0 (cmf:746, dmt:1228) goes back to the same byte when Open3D scales and rounds it.
  OBJ  `# Created by Open3D`, `# number of vertices: N`, `# number of triangles: M`, then N lines `v x y z r g b` -- coordinates in
       repr() form, the shortest text that reads back to the same f64, colours as repr(byte / 255.0) --, then M lines `f a b c`,
       1-based.  Every vertex is written, used or not: the triangles index the full array (cmf:734-735 says why).
Each writer writes `path + ".tmp"` and renames it, so a reader never sees half a file."""
from __future__ import annotations

import os

import numpy as np

PLY_HEADER = ("ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex {n}\n"
              "property double x\nproperty double y\nproperty double z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
PLY_RECORD = np.dtype([("xyz", "<f8", (3,)), ("rgb", "u1", (3,))])          # 27 bytes, packed


def _arrays(points, colors_u8, what):
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    c = np.asarray(colors_u8)
    if c.dtype != np.uint8:
        raise TypeError(f"{what}: colours must be uint8, got {c.dtype}")
    c = np.ascontiguousarray(c).reshape(-1, 3)
    if len(c) != len(p):
        raise ValueError(f"{what}: {len(p)} points and {len(c)} colours")
    return p, c


def _replace(path, data: bytes):
    tmp = str(path) + ".tmp"
    try:
        with open(tmp, "wb") as fh:
            fh.write(data)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def write_ply(path, points, colors_u8):
    p, c = _arrays(points, colors_u8, "write_ply")
    rec = np.empty(len(p), PLY_RECORD)
    rec["xyz"], rec["rgb"] = p, c
    _replace(path, PLY_HEADER.format(n=len(p)).encode("ascii") + rec.tobytes())


def read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n = next(int(l.split()[2]) for l in lines if l.startswith("element vertex "))
    if data[:end] != PLY_HEADER.format(n=n).encode("ascii"):
        raise ValueError(f"{path}: not a point cloud of this project's layout")
    if len(data) - end != n * PLY_RECORD.itemsize:
        raise ValueError(f"{path}: {len(data) - end} bytes of records for {n} vertices")
    rec = np.frombuffer(data, PLY_RECORD, n, end)
    return rec["xyz"].astype(np.float64), rec["rgb"].copy()


def write_obj(path, vertices, colors_u8, triangles):
    v, c = _arrays(vertices, colors_u8, "write_obj")
    t = np.ascontiguousarray(triangles, np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_obj: a triangle refers to a vertex that is not there")
    shade = [repr(k / 255.0) for k in range(256)]
    out = ["# Created by Open3D", f"# number of vertices: {len(v)}", f"# number of triangles: {len(t)}"]
    out += [f"v {x!r} {y!r} {z!r} {shade[r]} {shade[g]} {shade[b]}" for (x, y, z), (r, g, b) in zip(v.tolist(), c.tolist())]
    out += [f"f {a + 1} {b + 1} {d + 1}" for a, b, d in t.tolist()]
    _replace(path, ("\n".join(out) + "\n").encode("ascii"))


def read_obj(path):
    v, c, t = [], [], []
    with open(path, "r", encoding="ascii") as fh:
        for line in fh:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
                c.append([float(x) for x in w[4:7]])
            elif w[0] == "f":
                t.append([int(x) - 1 for x in w[1:4]])
            else:
                raise ValueError(f"{path}: unexpected line {line!r}")
    colors = np.rint(np.asarray(c, np.float64).reshape(-1, 3) * 255.0).astype(np.uint8)
    return np.asarray(v, np.float64).reshape(-1, 3), colors, np.asarray(t, np.int32).reshape(-1, 3)
