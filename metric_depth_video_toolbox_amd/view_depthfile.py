"""Device-side pieces of the reference's 3d_view_depthfile.py --render (3dv:133-258): a depth video drawn from a free camera.

The camera -- where it stands, what it looks at, the matrix a render takes for it --, the image, and the tool's loop over a file.

    centers(depth_rgb, params, renderer)       draw_mesh.get_center() of 3dv:231 for N frames, on the device (mdvt_view_centers)
    camera_position(x, y, z)                   3dv:239: the flags rounded to float32, then used in float64
    look_at_target(center, tx, ty, tz)         3dv:231-237: an exact -99.0 means "that coordinate of the centre"
    look_at_view(cam_pos, target)              the world-to-camera matrix V the project renders a view with (a decree, below)
    view_params(params, views)                 the frame parameter records of a view: T = V @ T_frame, has_T = 1
    render_view(depth_rgb, color_rgb, views, params, renderer)   one image per frame (mdvt_render_view_batch), holes in the key colour
    cam_look_at(cam_pos, target, up)           dmt:1618-1638 restated, for completeness; nothing renders with it
    run(depth_video, ...)                      the tool's --render loop on an .mkv file or a .npy frame dump -> <depth_video>_render.mkv / .npy
    python -m metric_depth_video_toolbox_amd.view_depthfile --depth_video X.mkv --xfov 45 --render [the reference's flags]

The centre is the mean of every transformed vertex of a frame; the sums run in NumPy's order (include/mdvt_view.h states it and why
that order and not Open3D's is the decree).  No CPU fallback.

The camera decree.  What Open3D makes of cam_look_at's matrix -- its rotation transposed, cam_pos with a negated z in the last
column, a last row that is not (0, 0, 0, 1) -- cannot be observed without Open3D.  The project takes the flags at their word: the
camera stands at --x --y --z and looks at the target; look_at_view is the matrix that says so, in the camera axes of the rest of the
path (x right, y down, z forward).

render_view draws ONE image per frame with one eye's work (the one-eye instantiations of the general kernels): what the left eye of
the stereo render gives with pupillary distance 0 and the composed matrix, except that holes keep the renderer's key colour (3dv:254
writes the render as it comes).  In points mode with remove_edges the parked vertices are not drawn, as in the stereo path (the
reference would draw them as one pixel at V (-0.2, -0.2, -0.2)); the centre still counts them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os

import numpy as np

from . import _lib

TARGET_FROM_CENTER = -99.0                              # 3dv:45-47, 232-237
DEFAULT_CAMERA = (2.0, 2.0, -4.0)                       # 3dv:42-44


def cam_look_at(cam_pos, target, up=(0.0, 1.0, 0.0)):
    """dmt:1618-1638 in float64, operation for operation (tests/golden/view_look_at.npz holds the reference's own results): forward,
    right and up as COLUMNS, cam_pos with its z negated in the last column, minus the axes' dot products with the TARGET in the last
    row.  Not a rigid world-to-camera matrix; see the module's text."""
    cam_pos, up = np.asarray(cam_pos), np.asarray(up, np.float64)
    f = np.array(np.asarray(target) - cam_pos, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(up, f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    return np.array([[r[0], u[0], f[0], cam_pos[0]],
                     [r[1], u[1], f[1], cam_pos[1]],
                     [r[2], u[2], f[2], -cam_pos[2]],
                     [-np.dot(r, target), -np.dot(u, target), -np.dot(f, target), 1.0]], dtype=float)


def camera_position(x=DEFAULT_CAMERA[0], y=DEFAULT_CAMERA[1], z=DEFAULT_CAMERA[2]):
    """3dv:239: np.array([x, y, z]).astype(np.float32) -- and float64 from there on."""
    return np.array([x, y, z]).astype(np.float32).astype(np.float64)


def needs_center(tx=TARGET_FROM_CENTER, ty=TARGET_FROM_CENTER, tz=TARGET_FROM_CENTER) -> bool:
    """Does the target take a coordinate of the centre?  With all three given the centres need not be computed."""
    return any(float(t) == TARGET_FROM_CENTER for t in (tx, ty, tz))


def look_at_target(center, tx=TARGET_FROM_CENTER, ty=TARGET_FROM_CENTER, tz=TARGET_FROM_CENTER):
    """3dv:231-237: the centre, with the coordinates that are not exactly -99.0 replaced by the flags'.  center may be None when
    needs_center() is False."""
    if center is None:
        if needs_center(tx, ty, tz):
            raise ValueError("a target coordinate of -99.0 takes the centre's: the centre is needed")
        center = (0.0, 0.0, 0.0)
    t = np.array(center, np.float64).reshape(3)
    for k, v in enumerate((tx, ty, tz)):
        if float(v) != TARGET_FROM_CENTER:
            t[k] = float(v)
    return t


def look_at_view(cam_pos, target):
    """The 4 x 4 world-to-camera matrix of a camera at cam_pos that looks at target, y down: in float64 and this order
    f = (t - p) / |t - p|, r = cross((0, 1, 0), f) / |.|, u = cross(f, r); rows [r, -r.p], [u, -u.p], [f, -f.p], (0, 0, 0, 1).
    p = 0, t = (0, 0, 1) gives the identity.  A target at the camera, or straight above or below it, has no such matrix."""
    p = np.asarray(cam_pos, np.float64).reshape(3)
    t = np.asarray(target, np.float64).reshape(3)
    f = t - p
    n = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
    if not n > 0.0:
        raise ValueError("the camera stands on its target")
    f = f / n
    r = np.array([f[2], 0.0, -f[0]])                    # cross((0, 1, 0), f) = (1 * f_z - 0 * f_y, 0 * f_x - 0 * f_z, 0 * f_y - 1 * f_x)
    n = np.sqrt(r[0] * r[0] + r[2] * r[2])
    if not n > 0.0:
        raise ValueError("the target lies straight above or below the camera: the view has no up direction")
    r = r / n
    u = np.array([f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]])
    V = np.zeros((4, 4), np.float64)
    for k, axis in enumerate((r, u, f)):
        V[k, :3] = axis
        V[k, 3] = -((axis[0] * p[0] + axis[1] * p[1]) + axis[2] * p[2])
    V[3, 3] = 1.0
    return V


def view_params(params, views):
    """The records a render takes for the views: a copy of each of `params` (one MdvtFrameParams or a sequence of N) with
    T = views[k] @ T_k (T_k the identity without has_T) as one NumPy product, has_T = 1 and no convergence.  views: [N, 4, 4]."""
    views = np.asarray(views, np.float64).reshape(-1, 4, 4)
    n = views.shape[0]
    if isinstance(params, _lib.MdvtFrameParams):
        params = [params] * n
    if len(params) != n:
        raise ValueError(f"need {n} frame parameter records, got {len(params)}")
    out = (_lib.MdvtFrameParams * n)()
    for k in range(n):
        C.memmove(C.byref(out[k]), C.byref(params[k]), C.sizeof(_lib.MdvtFrameParams))
        T = np.array([params[k].T[i] for i in range(16)], np.float64).reshape(4, 4) if params[k].has_T else np.eye(4)
        M = (views[k] @ T).reshape(16)
        for i in range(16):
            out[k].T[i] = M[i]
        out[k].has_T = 1
        out[k].convergence_angle = 0.0
    return out


def centers(depth_rgb, params, renderer, *, stream=None):
    """draw_mesh.get_center() (3dv:231) of N frames.  depth_rgb: uint8 CUDA [N, H, W, 3] or [H, W, 3] of the renderer's size (rows and
    frames may be padded); params: one MdvtFrameParams, a sequence of N or a packed array (K, depth_scale and the pose are read);
    renderer: the StereoRerenderer whose context supplies mode, remove_edges and max_depth.  Returns the float64 CUDA tensor [N, 3].
    Only enqueues, on `stream` (default: the current stream of the frames' device)."""
    import torch
    if depth_rgb.dim() == 3:
        depth_rgb = depth_rgb[None]
    if not depth_rgb.is_cuda or depth_rgb.dtype != torch.uint8 or depth_rgb.dim() != 4 or depth_rgb.shape[-1] != 3:
        raise ValueError("depth_rgb must be a uint8 CUDA tensor [N, H, W, 3]")
    N = int(depth_rgb.shape[0])
    if N < 1:
        raise ValueError("depth_rgb holds no frame")
    if tuple(depth_rgb.shape[1:3]) != (renderer.H, renderer.W):
        raise ValueError(f"depth frames are {int(depth_rgb.shape[2])}x{int(depth_rgb.shape[1])}, the renderer's {renderer.W}x{renderer.H}")
    if not (depth_rgb.stride(-1) == 1 and depth_rgb.stride(-2) == 3):
        raise ValueError("depth_rgb must have packed 3-byte pixels (rows and frames may be padded)")
    if depth_rgb.stride(1) < 3 * renderer.W or (N > 1 and depth_rgb.stride(0) < renderer.H * depth_rgb.stride(1)):
        raise ValueError(f"depth_rgb: rows or frames overlap (they may be padded, not folded: strides {tuple(depth_rgb.stride())})")
    if depth_rgb.device.index != renderer.device:
        raise ValueError(f"depth_rgb is on {depth_rgb.device}, the renderer on cuda:{renderer.device}")
    arr = renderer.pack_params(params, N)
    dev = depth_rgb.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    renderer.ctx.call("mdvt_view_centers", N, arr, depth_rgb.data_ptr(), depth_rgb.stride(1), depth_rgb.stride(0), out.data_ptr(),
                      _lib.stream_arg(dev, s))
    return out


WHITE = (255, 255, 255)                                 # 3dv:254: bg_color = (1, 1, 1)


def view_renderer(width, height, *, device=None, max_depth=100, render_as_pointcloud=False, remove_edges=False, cull=0,
                  key_rgb=WHITE, workspace_mib=0, subpixel_bits=0):
    """A StereoRerenderer set up as the viewer needs it: no baseline (depth scale 1 is the
    caller's: make_frame_params(..., master_xfov=xfov)), no edge points, and the
    background key of 3dv:254 (white) in place of the stereo tool's black."""
    from .stereo_rerender import StereoRerenderer
    r = StereoRerenderer(width, height, device=device, pupillary_distance=0, max_depth=max_depth, render_as_pointcloud=render_as_pointcloud,
                         remove_edges=remove_edges, dont_place_points_in_edges=True, cull=cull, workspace_mib=workspace_mib,
                         subpixel_bits=subpixel_bits)
    for k in range(3):
        r._cfg.key_rgb[k] = int(key_rgb[k])
    r.ctx.call("mdvt_set_config", C.byref(r._cfg))
    r.key_rgb = tuple(int(v) for v in key_rgb)
    return r


def render_view(depth_rgb, color_rgb, views, params, renderer, *, want_mask: bool = True, want_depth: bool = False,
                want_hole_counts: bool = False, stream=None):
    """3dv:254 for N frames: depth_rgb, color_rgb uint8 CUDA [N, H, W, 3] (or [H, W, 3]; rows and frames may be padded), views
    [N, 4, 4] world-to-camera matrices (look_at_view), params the frames' records (their poses are composed with the views by
    view_params).  Returns dict(rgb=[N, H, W, 3] u8 with the holes in the renderer's key colour, mask=[N, H, W] u8 (255 = hole),
    depth=[N, H, W] f32 (0 = background), hole_counts=[N] int32), the optional ones where asked for.  Only enqueues, on `stream`."""
    import torch
    single = depth_rgb.dim() == 3
    if single:
        depth_rgb, color_rgb = depth_rgb[None], color_rgb[None]
    N, H, W = int(depth_rgb.shape[0]), renderer.H, renderer.W
    for name, t in (("depth_rgb", depth_rgb), ("color_rgb", color_rgb)):
        if not t.is_cuda or t.dtype != torch.uint8 or tuple(t.shape) != (N, H, W, 3) or not (t.stride(-1) == 1 and t.stride(-2) == 3):
            raise ValueError(f"{name} must be a uint8 CUDA tensor [N, {H}, {W}, 3] with packed pixels")
        if t.stride(1) < 3 * W or (N > 1 and t.stride(0) < H * t.stride(1)):
            raise ValueError(f"{name}: rows or frames overlap (they may be padded, not folded: strides {tuple(t.stride())})")
        if t.device.index != renderer.device:
            raise ValueError(f"{name} is on {t.device}, the renderer on cuda:{renderer.device}")
    arr = view_params(renderer.pack_params(params, N), views)
    dev = depth_rgb.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    io = _lib.MdvtViewIO()
    io.depth_rgb, io.depth_pitch, io.depth_stride = depth_rgb.data_ptr(), depth_rgb.stride(1), depth_rgb.stride(0)
    io.color_rgb, io.color_pitch, io.color_stride = color_rgb.data_ptr(), color_rgb.stride(1), color_rgb.stride(0)
    with torch.cuda.stream(s):
        rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        io.rgb, io.rgb_pitch, io.rgb_stride = rgb.data_ptr(), 3 * W, 3 * W * H
        out = {"rgb": rgb[0] if single else rgb}
        if want_mask:
            mask = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
            io.mask, io.mask_pitch, io.mask_stride = mask.data_ptr(), W, W * H
            out["mask"] = mask[0] if single else mask
        if want_depth:
            z = torch.empty((N, H, W), dtype=torch.float32, device=dev)
            io.depth, io.zout_pitch, io.zout_stride = z.data_ptr(), 4 * W, 4 * W * H
            out["depth"] = z[0] if single else z
        if want_hole_counts:
            counts = torch.empty(N, dtype=torch.int32, device=dev)
            io.hole_counts = counts.data_ptr()
            out["hole_counts"] = counts[0] if single else counts
    renderer.ctx.call("mdvt_render_view_batch", N, arr, C.byref(io), _lib.stream_arg(dev, s))
    return out


# ------------------------------------------------------------------------------------------------
# the tool: 3dv:133-258 with --render
# ------------------------------------------------------------------------------------------------
REFUSED = {                                             # flag -> why the device path does not take it
    "render": "without --render the reference opens Open3D's interactive window (3dv:104-115): only the render to a video is built",
    "draw_frame": "--draw_frame opens Open3D's GUI on one frame (3dv:216-218)",
    "show_camera": "--show_camera draws an Open3D LineSet (3dv:170-176)",
    "background_ply": "--background_ply adds an Open3D point cloud to the scene (3dv:90-92)",
    "compressed": "--compressed writes avc1 (3dv:121-123): only the lossless FFV1 output is built",
    "mask_video": "--mask_video drops masked cells from the mesh (dmt:1326-1334), a render rule the oracle cannot express",
    "invert_mask": "--invert_mask belongs to --mask_video (dmt:1326-1334), a render rule the oracle cannot express",
}


def check_flags(*, render=True, draw_frame=-1, show_camera=False, background_ply=None, compressed=False, mask_video=None, invert_mask=False):
    """NotImplementedError, naming the reason, for what only Open3D's objects or another render rule could do."""
    if not render:
        raise NotImplementedError(REFUSED["render"])
    for name, on in (("draw_frame", draw_frame != -1), ("show_camera", show_camera), ("background_ply", background_ply is not None),
                     ("compressed", compressed), ("mask_video", mask_video is not None), ("invert_mask", invert_mask)):
        if on:
            raise NotImplementedError(REFUSED[name])


def run(depth_video, color_video=None, *, xfov=None, yfov=None, max_depth=100, render=True, render_as_pointcloud=False, remove_edges=False,
        max_frames=-1, transformation_file=None, transformation_lock_frame=0, x=DEFAULT_CAMERA[0], y=DEFAULT_CAMERA[1], z=DEFAULT_CAMERA[2],
        tx=TARGET_FROM_CENTER, ty=TARGET_FROM_CENTER, tz=TARGET_FROM_CENTER, batch=8, video_decoder="host", video_encoder="host", device=None,
        draw_frame=-1, show_camera=False, background_ply=None, compressed=False, mask_video=None, invert_mask=False):
    """The frame loop of 3dv:133-258 with --render on `.mkv` files (-> `<depth_video>_render.mkv` at the depth video's frame rate) or
    `.npy` frame dumps (-> `<depth_video>_render.npy`), written under a `_tmp_render` name and renamed when complete.  Without a
    colour video the depth video's own bytes are the colour (3dv:150).  Depth scale 1, white background.  max_frames = N writes N
    frames (the reference's off-by-one is dropped).  Per batch the centres are read back once (24 bytes a frame) -- not at all when
    --tx --ty --tz are all given --, the views are built on the host and the batch is rendered.  Returns the output path."""
    import torch
    from . import distributed as D
    from .clip_io import ClipInputs, ClipOutput, check_video_decoder, check_video_encoder, video_parts
    from .stereo_rerender import make_frame_params
    check_flags(render=render, draw_frame=draw_frame, show_camera=show_camera, background_ply=background_ply, compressed=compressed,
                mask_video=mask_video, invert_mask=invert_mask)
    if xfov is None and yfov is None:
        raise ValueError("Either --xfov or --yfov is required.")                                  # 3dv:54-56
    if max_frames == 0:
        raise ValueError("max_frames = 0 writes nothing: ask for -1 (all) or a positive count")
    with ClipInputs() as inp:
        depth = inp.open(depth_video, "depth_video", Exception("input video does not exist"))                                       # 3dv:62-63
        color = None if color_video is None else inp.open(color_video, "color_video", Exception("input color_video does not exist"))    # 3dv:67-68
        video = bool(video_parts(depth))
        check_video_decoder(video_decoder, video)
        check_video_encoder(video_encoder, video)
        if depth.ndim != 4 or depth.shape[-1] != 3 or depth.dtype != np.uint8:
            raise ValueError(f"{depth_video}: uint8 [N, H, W, 3] expected")
        if color is not None and tuple(color.shape[1:]) != tuple(depth.shape[1:]):
            raise ValueError("color image and depth image need to have same width and height")     # 3dv:148
        H, W = int(depth.shape[1]), int(depth.shape[2])
        n = depth.shape[0] if max_frames < 0 else min(depth.shape[0], max_frames)
        if color is not None:
            n = min(n, color.shape[0])
        T = None
        if transformation_file is not None:
            if not os.path.isfile(transformation_file):
                raise Exception("input transformation_file does not exist")                        # 3dv:79-80
            with open(transformation_file) as fh:
                T = D.rebase_on_lock_frame(json.load(fh), transformation_lock_frame)               # 3dv:84-88
            if len(T) < n:
                raise ValueError("transformation file has fewer entries than frames")
        cam = camera_position(x, y, z)
        want_centers = needs_center(tx, ty, tz)
        ext = ".mkv" if video else ".npy"
        tmp, final = depth_video + "_tmp_render" + ext, depth_video + "_render" + ext              # 3dv:125
        fps = (video_parts(depth)[0][0].fps or 30.0) if video else None
        batch = max(1, int(batch))
        inp.on_device(torch.device("cuda", torch.cuda.current_device() if device is None else device), video_decoder, video_encoder)
        r = view_renderer(W, H, device=inp.dev.index, max_depth=max_depth, render_as_pointcloud=render_as_pointcloud, remove_edges=remove_edges)
        try:
            with ClipOutput(tmp, final, n, (H, W, 3), fps, video_encoder, inp.ctx) as out, torch.cuda.device(inp.dev):
                for a in range(0, n, batch):
                    b = min(a + batch, n)
                    d_depth = inp.fetch(depth, a, b)
                    d_color = d_depth if color is None else inp.fetch(color, a, b)
                    xf = xfov if xfov is not None else float(np.rad2deg(2 * np.arctan2(W, 2 * (H / (2.0 * np.tan(np.deg2rad(yfov) / 2.0))))))
                    params = [make_frame_params(W, H, xfov, yfov, master_xfov=xf, pupillary_distance=0,
                                                transformation=None if T is None else np.asarray(T[k], np.float64)) for k in range(a, b)]
                    cen = centers(d_depth, params, r).cpu().numpy() if want_centers else [None] * (b - a)
                    views = np.stack([look_at_view(cam, look_at_target(cen[k], tx, ty, tz)) for k in range(b - a)])
                    out.store(render_view(d_depth, d_color, views, params, r, want_mask=False)["rgb"], a)
        finally:
            r.close()
    return final


def build_parser():
    p = argparse.ArgumentParser(description="Take a rgb encoded depth video and a color video, and render it as 3D from a free camera")
    p.add_argument("--depth_video", type=str, required=True, help="video file to use as input (.mkv, or a .npy frame dump)")
    p.add_argument("--color_video", type=str, required=False, help="video file to use as color input")
    p.add_argument("--xfov", type=int, required=False, help="fov in deg in the x-direction")
    p.add_argument("--yfov", type=int, required=False, help="fov in deg in the y-direction")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses")
    p.add_argument("--render", action="store_true", help="Render to video instead of GUI (required here: the GUI is not built)")
    p.add_argument("--render_as_pointcloud", action="store_true", help="Render as point cloud instead of as mesh")
    p.add_argument("--remove_edges", action="store_true", help="Tries to remove edges that was not visible in image")
    p.add_argument("--show_camera", action="store_true", help="refused: an Open3D object")
    p.add_argument("--background_ply", type=str, required=False, help="refused: an Open3D object")
    p.add_argument("--mask_video", type=str, required=False, help="refused: a render rule that is not built")
    p.add_argument("--invert_mask", action="store_true", help="refused with --mask_video")
    p.add_argument("--compressed", action="store_true", help="refused: only FFV1 output is built")
    p.add_argument("--draw_frame", default=-1, type=int, help="refused: the GUI")
    p.add_argument("--max_frames", default=-1, type=int, help="quit after max_frames nr of frames")
    p.add_argument("--transformation_file", type=str, required=False, help="file with scene transformations from the aligner")
    p.add_argument("--transformation_lock_frame", default=0, type=int, help="the frame that the transformation will use as a base")
    p.add_argument("--x", default=DEFAULT_CAMERA[0], type=float, help="camera x in meters")
    p.add_argument("--y", default=DEFAULT_CAMERA[1], type=float, help="camera y in meters")
    p.add_argument("--z", default=DEFAULT_CAMERA[2], type=float, help="camera z in meters")
    p.add_argument("--tx", default=TARGET_FROM_CENTER, type=float, help="camera target x in meters (-99.0: the centre's)")
    p.add_argument("--ty", default=TARGET_FROM_CENTER, type=float, help="camera target y in meters (-99.0: the centre's)")
    p.add_argument("--tz", default=TARGET_FROM_CENTER, type=float, help="camera target z in meters (-99.0: the centre's)")
    p.add_argument("--batch", default=8, type=int, help="not a reference flag: frames per device call")
    p.add_argument("--video_decoder", choices=("host", "device", "device_all"), default="host", help="not a reference flag: where .mkv inputs are decoded")
    p.add_argument("--video_encoder", choices=("host", "device"), default="host", help="not a reference flag: where the .mkv output is encoded")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    out = run(a.depth_video, a.color_video, xfov=a.xfov, yfov=a.yfov, max_depth=a.max_depth, render=a.render,
              render_as_pointcloud=a.render_as_pointcloud, remove_edges=a.remove_edges, max_frames=a.max_frames,
              transformation_file=a.transformation_file, transformation_lock_frame=a.transformation_lock_frame, x=a.x, y=a.y, z=a.z,
              tx=a.tx, ty=a.ty, tz=a.tz, batch=a.batch, video_decoder=a.video_decoder, video_encoder=a.video_encoder,
              draw_frame=a.draw_frame, show_camera=a.show_camera, background_ply=a.background_ply, compressed=a.compressed,
              mask_video=a.mask_video, invert_mask=a.invert_mask)
    print(f"Done. Wrote: {out}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
