"""Device-side mirror of the reference's relative-depth producers (video_metric_convert.py:17-41, 101-149 for Video-Depth-Anything,
depthcrafter_video.py:19-43, 200-252 for DepthCrafter, geometrycrafter_video.py:244): a relative inverse depth tensor becomes the
metric 16-bit RGB depth video without leaving the GPU.  The fit's five float32 sums follow NumPy's order of summation, the inverse is
one correctly rounded division, the resize restates cv2.resize(INTER_LINEAR) (include/mdvt_metric_align.h states all three; the
kernels are csrc/mdvt_metric_align.hip).  No CPU fallback.

    compute_scale_and_shift_full(prediction, target, mask)    vmc:17-41 on device tensors -> Fit (8 floats on the device)
    metric_depth_codes(relative, fit, max_depth, style=...)   vmc:136-142 / dcv:236-243 + dfh:125-161 -> uint8 [N, H', W', 3]
    convert(relative, reference_depth, engine=...)            the driver lines around them (vmc:107-125, dcv:203-225)
    python -m metric_depth_video_toolbox_amd.video_metric_convert --color_video x.mkv --relative_depth rel.npy
           (--depth_video ref.mkv | --metric_depth ref.npy) [--max_depth 100] [--max_frames N] [--engine vda|depthcrafter]
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import _lib, video_io
from .clip_io import VIDEO_DECODERS, ClipInputs, ClipOutput, check_video_decoder, check_video_encoder

ENGINES = {"vda": 0, "depthcrafter": 1}                  # engine -> reconstruction style (include/mdvt_metric_align.h)
FIT_FRAMES = 32                                          # vmc:107


class Fit:
    """The result of a fit, on the device: .values is the float32 CUDA tensor a_00, a_01, a_11, b_0, b_1, scale, shift, det."""

    def __init__(self, values):
        self.values = values

    def scale_shift(self):
        """(scale, shift) as np.float32: reads back, so it waits for the fit."""
        v = self.values.cpu().numpy()
        return v[5], v[6]

    def numpy(self):
        return self.values.cpu().numpy()


def _planes(t, name: str, dtypes, like=None):
    """-> the tensor as [N, H, W] with unit column stride (rows and frames may be strided); ValueError for anything else."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes or t.dim() not in (2, 3):
        raise ValueError(f"{name} must be a CUDA tensor [N, H, W] or [H, W] of {' or '.join(str(d) for d in dtypes)}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.numel() == 0:
        raise ValueError(f"{name} holds no value")
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{name} must have unit column stride (rows and frames may be padded)")
    if t.stride(1) < t.shape[2] or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * t.stride(1)):
        raise ValueError(f"{name}: rows or frames overlap")
    if like is not None:
        if tuple(t.shape) != tuple(like.shape):
            raise ValueError(f"{name} is {tuple(t.shape)}, the prediction {tuple(like.shape)}")
        if t.device != like.device:
            raise ValueError(f"{name} and the prediction are on different devices")
    return t


def compute_scale_and_shift_full(prediction, target, mask=None, *, target_is_depth: bool = False, stream=None) -> Fit:
    """vmc:17-41: the least-squares scale and shift with target ~ scale * prediction + shift over all values of the float32 CUDA
    tensors [N, H, W] (or [H, W]; rows and frames may be strided), under an optional bool / uint8 mask of the same shape (a byte v
    counts as float32(v)).  target_is_depth: the target tensor holds metric depth and the library takes float32(1) / depth itself.
    Returns the Fit on the device; only enqueues, on `stream` (default: the current stream of the prediction's device)."""
    import torch
    p = _planes(prediction, "prediction", (torch.float32,))
    t = _planes(target, "target", (torch.float32,), p)
    m = None
    if mask is not None:
        m = _planes(mask, "mask", (torch.bool, torch.uint8), p)
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
    N, H, W = (int(v) for v in p.shape)
    if N * H * W >= 1 << 31:
        raise ValueError(f"{N} x {H} x {W} values are more than one fit takes (2^31 - 1)")
    dev = p.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        out = torch.empty(8, dtype=torch.float32, device=dev)
    _lib.shared_context(dev).call(                          # (the render size is irrelevant here too)
        "mdvt_scale_shift_fit", W, H, N, p.data_ptr(), 4 * p.stride(1), 4 * p.stride(0), t.data_ptr(), 4 * t.stride(1), 4 * t.stride(0),
        int(bool(target_is_depth)), m.data_ptr() if m is not None else None, m.stride(1) if m is not None else 0,
        m.stride(0) if m is not None else 0, out.data_ptr(), _lib.stream_arg(dev, s))
    return Fit(out)


def _check_codes_args(max_depth, style, out_size):
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    if style not in (0, 1):
        raise ValueError(f"style must be 0 (video_metric_convert) or 1 (depthcrafter_video), got {style!r}")
    if out_size is not None:
        if len(out_size) != 2 or int(out_size[0]) < 1 or int(out_size[1]) < 1:
            raise ValueError(f"out_size must be (width, height) with both at least 1, got {out_size!r}")


def metric_depth_codes(relative, fit, max_depth, *, style: int = 0, out_size=None, bgr: bool = False, want_depth: bool = False,
                       out=None, stream=None):
    """Relative inverse depth planes (float32 CUDA [N, H, W] or [H, W]) -> the uint8 [N, H', W', 3] 16-bit depth codes of
    1 / (relative * scale + shift) (R, G, B order, or B, G, R with bgr=True), resized to out_size = (width, height) where that
    differs.  fit: a Fit, or a float32 CUDA tensor whose elements 5 and 6 are scale and shift (8 floats), or just the two.
    style 0: negative depths become max_depth (vmc:136-142); style 1: depthcrafter_video.py:236-243.  want_depth: also the float32
    [N, H', W'] planes of the coded (clipped) depth.  out: the codes' tensor to fill.  Only enqueues, on `stream`."""
    import torch
    _check_codes_args(max_depth, style, out_size)
    x = _planes(relative, "relative", (torch.float32,))
    N, H, W = (int(v) for v in x.shape)
    ow, oh = (W, H) if out_size is None else (int(out_size[0]), int(out_size[1]))
    v = fit.values if isinstance(fit, Fit) else fit
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or v.dim() != 1 or v.numel() not in (2, 8) \
            or not v.is_contiguous() or _lib.device_index(v.device) != _lib.device_index(x.device):
        raise ValueError("fit must be a Fit, or a contiguous float32 CUDA tensor of 8 floats (a fit's) or of 2 (scale, shift)")
    ss = v[5:7] if v.numel() == 8 else v
    dev = x.device
    s = torch.cuda.current_stream(dev) if stream is None else stream
    if out is not None:
        from . import ffv1_device
        ffv1_device.check_out(out, N, oh, ow)
        if _lib.device_index(out.device) != _lib.device_index(dev):
            raise ValueError(f"out is on {out.device}, the relative depth on {dev}")
    with torch.cuda.stream(s):
        codes = torch.empty((N, oh, ow, 3), dtype=torch.uint8, device=dev) if out is None else out
        depth = torch.empty((N, oh, ow), dtype=torch.float32, device=dev) if want_depth else None
    _lib.shared_context(dev).call(
        "mdvt_metric_depth_codes", W, H, N, x.data_ptr(), 4 * x.stride(1), 4 * x.stride(0), ss.data_ptr(), int(style), float(max_depth), ow, oh,
        codes.data_ptr(), codes.stride(1), codes.stride(0), int(bool(bgr)),
        depth.data_ptr() if want_depth else None, 4 * ow, 4 * ow * oh, _lib.stream_arg(dev, s))
    return (codes, depth) if want_depth else codes


def _decode_reference(ref, max_depth):
    """An RGB-coded reference [N, H, W, 3] uint8 -> float32 [N, H, W] metres (dfh:99, the existing decode)."""
    import torch
    from .depth_frames_helper import decode_rgb_depth_frame
    out = torch.empty(tuple(ref.shape[:3]), dtype=torch.float32, device=ref.device)
    for k in range(ref.shape[0]):
        decode_rgb_depth_frame(ref[k].contiguous(), max_depth, True, out=out[k])
    return out


def fit_reference(relative, reference_depth, max_depth=100, *, engine: str = "vda") -> Fit:
    """The driver lines in front of the fit, on device tensors.  reference_depth: float32 [M, H, W] metres, or the RGB-coded
    uint8 [M, H, W, 3] of a depth video.  "vda" (vmc:107-125): the first min(32, N, M) frames, target 1 / depth (a depth of 0 gives
    inf, as in the reference).  "depthcrafter" (dcv:203-225): the first min(N, M) frames without those whose reference is all zero
    (one read-back of M flags), zeros set to max_depth."""
    import torch
    if engine not in ENGINES:
        raise ValueError(f"engine must be one of {tuple(ENGINES)}, got {engine!r}")
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    x = _planes(relative, "relative", (torch.float32,))
    ref = reference_depth
    if isinstance(ref, torch.Tensor) and ref.dtype == torch.uint8 and ref.dim() == 4 and ref.shape[-1] == 3 and ref.is_cuda:
        if tuple(ref.shape[1:3]) != tuple(x.shape[1:]):
            raise ValueError(f"the reference frames are {ref.shape[2]}x{ref.shape[1]}, the relative depth {x.shape[2]}x{x.shape[1]}")
        n = min(int(ref.shape[0]), int(x.shape[0]), FIT_FRAMES if engine == "vda" else 1 << 30)
        if n < 1:
            raise ValueError("reference_depth holds no frame")
        ref = _decode_reference(ref[:n], max_depth)
    else:
        ref = _planes(ref, "reference_depth", (torch.float32,))
        if tuple(ref.shape[1:]) != tuple(x.shape[1:]) or ref.device != x.device:
            raise ValueError(f"the reference planes are {tuple(ref.shape[1:])}, the relative depth {tuple(x.shape[1:])} (one device)")
        n = min(int(ref.shape[0]), int(x.shape[0]), FIT_FRAMES if engine == "vda" else 1 << 30)
        ref = ref[:n]
    src = x[:n]
    if engine == "depthcrafter":
        used = (ref != 0).flatten(1).any(1)                                                  # dcv:208
        if not bool(used.all()):
            keep = torch.nonzero(used).flatten()
            if keep.numel() == 0:
                raise ValueError("every reference frame is all zero: nothing to fit against")
            ref, src = ref[keep], src[keep].contiguous()
        ref = torch.where(ref == 0, torch.tensor(float(max_depth), dtype=torch.float32, device=ref.device), ref)      # dcv:212
    return compute_scale_and_shift_full(src, ref, target_is_depth=True)


def convert(relative, reference_depth, max_depth=100, *, engine: str = "vda", out_size=None, bgr: bool = False,
            want_depth: bool = False, fit=None):
    """relative [N, H, W] float32 CUDA + a metric reference (fit_reference) -> the depth codes uint8 [N, H', W', 3] that
    `<color_video>_depth.mkv` holds and StereoRerenderer.render takes (and the depth planes with want_depth).  fit: a Fit made
    earlier (a clip converted batch by batch fits once, on its first frames)."""
    if fit is None:
        fit = fit_reference(relative, reference_depth, max_depth, engine=engine)
    elif engine not in ENGINES:
        raise ValueError(f"engine must be one of {tuple(ENGINES)}, got {engine!r}")
    return metric_depth_codes(relative, fit, max_depth, style=ENGINES[engine], out_size=out_size, bgr=bgr, want_depth=want_depth)


def output_paths(color_video: str):
    """(tmp, final): vmc:146-147."""
    return color_video + "_tmp_depth.mkv", color_video + "_depth.mkv"


def run(color_video: str, relative_depth: str, depth_video=None, metric_depth=None, max_depth=100, *, max_frames: int = -1,
        engine: str = "vda", batch: int = 16, video_encoder: str = "host", video_decoder: str = "host") -> str:
    """The script: relative_depth (a float32 [N, h, w] .npy dump, where the reference runs the model) is fitted against the RGB-coded
    depth_video (.mkv or a uint8 frame dump) or the float32 metric_depth dump, and `<color_video>_depth.mkv` is written at the
    colour video's size and frame rate (tmp -> rename, vmc:146-149).  Returns its path."""
    import torch
    if engine not in ENGINES:
        raise ValueError(f"engine must be one of {tuple(ENGINES)}, got {engine!r}")
    if not (float(max_depth) > 0):
        raise ValueError("max_depth must be > 0")
    if (depth_video is None) == (metric_depth is None):
        raise ValueError("give exactly one of --depth_video (RGB-coded reference) and --metric_depth (float32 dump)")
    check_video_encoder(video_encoder, True)
    coded = depth_video is not None
    ref_path = depth_video if coded else metric_depth
    check_video_decoder(video_decoder, coded and video_io.is_matroska(depth_video))
    for path, what in ((color_video, "Color video"), (relative_depth, "Relative depth")):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{what} not found: {path}")
    if not video_io.is_matroska(color_video):
        raise ValueError(f"{color_video}: --color_video must be an .mkv file (its size and frame rate are the output's)")
    rel = np.load(relative_depth, mmap_mode="r")
    if rel.ndim != 3 or rel.dtype != np.float32:
        raise ValueError(f"{relative_depth}: float32 [N, h, w] expected")
    tmp, final = output_paths(color_video)
    with ClipInputs() as inp:
        ref = inp.open(ref_path, "depth_video", FileNotFoundError(f"Reference depth not found: {ref_path}"))
        if coded and not (ref.ndim == 4 and ref.shape[3] == 3 and ref.dtype == np.uint8):
            raise ValueError(f"{ref_path}: uint8 [N, H, W, 3] expected")
        if not coded and not (ref.ndim == 3 and ref.dtype == np.float32):
            raise ValueError(f"{ref_path}: float32 [N, h, w] expected")
        if tuple(ref.shape[1:3]) != tuple(rel.shape[1:3]):
            raise ValueError(f"The reference depth is {ref.shape[2]}x{ref.shape[1]}, the relative depth {rel.shape[2]}x{rel.shape[1]}: "
                             "this build does not resize reference frames (the reference resizes RGB-coded frames, which is not restated)")
        with video_io.VideoReader(color_video) as cv:
            W, H, fps = cv.width, cv.height, cv.fps or 30.0
        n = rel.shape[0] if max_frames < 0 else min(rel.shape[0], max_frames)
        if n < 1:
            raise ValueError("no frame to convert")
        n_fit = min(n, ref.shape[0], FIT_FRAMES if engine == "vda" else n)
        if n_fit < 1:
            raise ValueError(f"{ref_path} holds no frame")
        batch = max(1, int(batch))
        inp.on_device(torch.device("cuda", torch.cuda.current_device()), video_decoder, video_encoder)
        dev = inp.dev
        with torch.cuda.device(dev):
            d_rel = torch.from_numpy(np.ascontiguousarray(rel[:n_fit])).to(dev)
            d_ref = inp.fetch(ref, 0, n_fit) if coded else torch.from_numpy(np.ascontiguousarray(ref[:n_fit])).to(dev)
            fit = fit_reference(d_rel, d_ref, max_depth, engine=engine)
            scale, shift = fit.scale_shift()
            print("scale:", scale, "shift:", shift)                                          # vmc:129
            with ClipOutput(tmp, final, n, (H, W, 3), fps, video_encoder, inp.ctx) as out:
                for a in range(0, n, batch):
                    d_rel = torch.from_numpy(np.ascontiguousarray(rel[a:min(a + batch, n)])).to(dev)
                    out.store(metric_depth_codes(d_rel, fit, max_depth, style=ENGINES[engine], out_size=(W, H)), a)
    return final


def build_parser():
    p = argparse.ArgumentParser(description="Relative (video-consistent) depth to a metric depth video")
    p.add_argument("--color_video", type=str, required=True, help="the colour video (.mkv): the output takes its size, frame rate and name")
    p.add_argument("--relative_depth", type=str, required=True,
                   help="not a reference flag: the model's relative inverse depth, a float32 [N, h, w] .npy dump (stands where the model stands)")
    p.add_argument("--depth_video", type=str, required=False, help="RGB-coded metric reference depth video (.mkv, or a uint8 .npy frame dump)")
    p.add_argument("--metric_depth", type=str, required=False, help="not a reference flag: metric reference depth as a float32 [M, h, w] .npy dump")
    p.add_argument("--max_depth", default=100, type=int, help="the max depth that the video uses")
    p.add_argument("--max_frames", default=-1, type=int, help="quit after max_frames nr of frames")
    p.add_argument("--engine", choices=tuple(ENGINES), default="vda",
                   help="whose driver lines and clean-up rule: vda (video_metric_convert.py) or depthcrafter (depthcrafter_video.py)")
    p.add_argument("--batch", default=16, type=int, help="not a reference flag: frames per device call")
    p.add_argument("--video_encoder", choices=("host", "device"), default="host",
                   help="not a reference flag: where the .mkv output is FFV1-encoded -- 'host' (default) or 'device' (the same bytes)")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="not a reference flag: where an .mkv --depth_video is FFV1-decoded -- 'host' (default), 'device' or 'device_all' "
                        "(the same bytes; 'device_all' also takes Golomb-Rice and inter-coded FFV1, FFmpeg's default, to the GPU)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    out = run(args.color_video, args.relative_depth, args.depth_video, args.metric_depth, args.max_depth, max_frames=args.max_frames,
              engine=args.engine, batch=args.batch, video_encoder=args.video_encoder, video_decoder=args.video_decoder)
    print(f"saved: {out}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
