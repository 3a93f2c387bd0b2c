"""The device wrappers of tools/export_depth_geometry.py: the functions that hand a tensor's address to the two entry points of
include/mdvt_geometry.h.  Both entry points take the frame size from the context, not from an argument, so the frames must have the
size the context was made for and lie on its GPU; a tensor that does not is refused before the library sees an address
(tests/binding_contract.py holds enqueue_export and grey_batch to their records).  torch is imported inside the functions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def frame_params(K, transforms):
    """MdvtFrameParams records of a batch: K, depth scale 1, the pose where there is one."""
    arr = (_lib.MdvtFrameParams * len(transforms))()
    for k, T in enumerate(transforms):
        for i, v in enumerate(np.asarray(K, np.float64).reshape(9)):
            arr[k].K[i] = arr[k].Krender[i] = v
        arr[k].depth_scale = 1.0
        if T is not None:
            arr[k].has_T = 1
            for i, v in enumerate(np.asarray(T, np.float64).reshape(16)):
                arr[k].T[i] = v
    return arr


def _context_frames(ctx, name, t, B=None):
    """A contiguous uint8 CUDA [B, H, W, 3] batch of the context's size on the context's GPU -> B."""
    import torch
    _lib.check_tensor(name, t, torch.uint8, (B, ctx.H, ctx.W, 3), contiguous=True)
    if t.device.index != ctx.device:
        raise ValueError(f"{name} is on {t.device}, the context on cuda:{ctx.device}")
    if t.shape[0] < 1:
        raise ValueError(f"{name} holds no frame: shape {tuple(t.shape)}")
    return int(t.shape[0])


def enqueue_export(ctx, d_depth, d_color, K, transforms, *, max_depth, remove_edges, decode=0, want_ply=True, want_obj=True, stream=None):
    """One call of mdvt_export_geometry_batch on contiguous uint8 CUDA [B, H, W, 3] depth and colour frames of the context's size ->
    the device tensors (counts int32 [B, 2] = (U, M), vertices float64 [B, H W, 3], triangles int32 [B, 2 (H - 1) (W - 1), 3],
    points float64 [B, H W, 3], point_rgb uint8 [B, H W, 3]); vertices and triangles are None without want_obj, points and point_rgb
    without want_ply.  Of a frame's triangles the first M entries are written, of its points and point_rgb the first U.  Only
    enqueues, on `stream`."""
    import torch
    B = _context_frames(ctx, "depth", d_depth)
    _context_frames(ctx, "color", d_color, B)
    if len(transforms) != B:
        raise ValueError(f"transforms must hold one entry per frame ({B}), got {len(transforms)}")
    H, W = ctx.H, ctx.W
    N, ncell, dev = W * H, (W - 1) * (H - 1), d_depth.device
    opts = _lib.MdvtGeometryOpts(decode=int(decode), remove_edges=int(bool(remove_edges)), max_depth=float(max_depth))
    io = _lib.MdvtGeometryIO()
    io.depth_rgb, io.depth_pitch, io.depth_stride = d_depth.data_ptr(), 3 * W, 3 * W * H
    io.color_rgb, io.color_pitch, io.color_stride = d_color.data_ptr(), 3 * W, 3 * W * H
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    io.counts = counts.data_ptr()
    vertices = triangles = points = point_rgb = None
    if want_obj:
        vertices = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
        triangles = torch.empty((B, 2 * ncell, 3), dtype=torch.int32, device=dev)
        io.vertices, io.vertices_stride = vertices.data_ptr(), 24 * N
        io.triangles, io.triangles_stride = triangles.data_ptr(), 24 * ncell
    if want_ply:
        points = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
        point_rgb = torch.empty((B, N, 3), dtype=torch.uint8, device=dev)
        io.points, io.points_stride = points.data_ptr(), 24 * N
        io.point_rgb, io.point_rgb_stride = point_rgb.data_ptr(), 3 * N
    ctx.call("mdvt_export_geometry_batch", B, frame_params(K, transforms), C.byref(opts), C.byref(io), _lib.stream_arg(dev, stream))
    return counts, vertices, triangles, points, point_rgb


def export_batch(ctx, d_depth, d_color, K, transforms, *, max_depth, remove_edges, decode=0, want_ply=True, want_obj=True, stream=None):
    """enqueue_export and its read-back -> per frame a dict of host arrays: points, point_rgb (want_ply), vertices, triangles
    (want_obj), counts (U, M).  The lists come back by their counts: counts first, then U or M entries."""
    counts, vertices, triangles, points, point_rgb = enqueue_export(ctx, d_depth, d_color, K, transforms, max_depth=max_depth,
                                                                    remove_edges=remove_edges, decode=decode, want_ply=want_ply,
                                                                    want_obj=want_obj, stream=stream)
    host_counts = counts.cpu().numpy()
    out = []
    for k in range(len(host_counts)):
        U, M = int(host_counts[k, 0]), int(host_counts[k, 1])
        f = {"counts": (U, M)}
        if want_ply:
            f["points"], f["point_rgb"] = points[k, :U].cpu().numpy(), point_rgb[k, :U].cpu().numpy()
        if want_obj:
            f["vertices"], f["triangles"] = vertices[k].cpu().numpy(), triangles[k, :M].cpu().numpy()
        out.append(f)
    return out


def grey_batch(ctx, d_depth, *, max_depth, bits, stream=None):
    """mdvt_depth_grey_batch on contiguous uint8 CUDA [B, H, W, 3] frames of the context's size -> CUDA int16 [B, H, W] holding the
    uint16 bit patterns (bits 16: view the host copy as np.uint16) or uint8 [B, H, W, 3] (bits 8).  Only enqueues, on `stream`."""
    import torch
    B, H, W = _context_frames(ctx, "depth", d_depth), ctx.H, ctx.W
    out = torch.empty((B, H, W) if bits == 16 else (B, H, W, 3), dtype=torch.int16 if bits == 16 else torch.uint8, device=d_depth.device)
    row = 2 * W if bits == 16 else 3 * W
    ctx.call("mdvt_depth_grey_batch", B, d_depth.data_ptr(), 3 * W, 3 * W * H, float(max_depth), int(bits), out.data_ptr(), row, row * H,
             _lib.stream_arg(d_depth.device, stream))
    return out
