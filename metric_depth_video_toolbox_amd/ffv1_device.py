"""FFV1 packets of device frames (mdvt_encode_video_frames): byte for byte those of video_io.encode_frame, without copying the raw
frames to the host.  A frame the device could not code (a slice past its capacity, or a packet past the packet buffer) is
re-encoded on the host, which gives the same bytes, or refuses the frame as the host encoder refuses it."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib

OVERFLOW = 0xFFFFFFFF        # d_sizes flag: a slice passed its capacity, or the packet the buffer: re-encode on the host
TOO_LARGE = 0xFFFFFFFE       # d_sizes flag: a slice of 2^24 bytes or more (the host encoder refuses the frame)


def check_frames(frames, slices) -> tuple:
    """-> (N, H, W, channels) of a (N, H, W, 3) or (N, H, W) uint8 CUDA tensor; ValueError for anything else."""
    import torch
    if not isinstance(frames, torch.Tensor):
        raise ValueError("frames must be a torch.Tensor on a CUDA device")
    if frames.dtype != torch.uint8:
        raise ValueError(f"frames must be uint8, got {frames.dtype}")
    if frames.dim() == 4 and frames.shape[3] == 3:
        ch = 3
    elif frames.dim() == 3:
        ch = 1
    else:
        raise ValueError(f"frames must be (N, H, W, 3) or (N, H, W), got {tuple(frames.shape)}")
    if not frames.is_cuda:
        raise ValueError("frames must be on a CUDA device")
    N, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f"empty frames {tuple(frames.shape)}")
    nh, nv = int(slices[0]), int(slices[1])
    if nh < 1 or nv < 1 or nh > W or nv > H or nh * nv > 1024:
        raise ValueError(f"slices {slices} for {W} x {H}: each >= 1 and at most the frame's width / height, product <= 1024")
    return N, H, W, ch


def slice_capacity_bytes(W: int, H: int, slices, slice_capacity: int = 0) -> int:
    """The payload bytes a slice may take on the device (include/mdvt.h): slice_capacity, or 0 = twice the largest slice's raw
    bytes + 4096; at most 2^24 - 1 (the 24-bit slice size)."""
    nh, nv = int(slices[0]), int(slices[1])
    max_raw = -(-W // nh) * -(-H // nv) * 3
    cap = int(slice_capacity) if slice_capacity else 2 * max_raw + 4096
    return min(cap, (1 << 24) - 1)


def packet_capacity_bytes(W: int, H: int, slices, slice_capacity: int = 0) -> int:
    """The largest packet the device writes for one frame: every slice at its capacity + its 8 trailer bytes.  A packet buffer of
    n_frames times this never flags a frame for lack of room (only a slice past its own capacity is flagged)."""
    return int(slices[0]) * int(slices[1]) * (slice_capacity_bytes(W, H, slices, slice_capacity) + 8)


class PendingPackets:
    """The device side of one encode: the packet buffer, offsets and sizes, filled on the stream the encode was enqueued on
    (`done` is recorded there behind it)."""

    def __init__(self, frames, slices, bgr, packets, offsets, sizes, done):
        self.frames, self.slices, self.bgr = frames, slices, bgr
        self.packets, self.offsets, self.sizes, self.done = packets, offsets, sizes, done
        self.host_frames = 0                  # frames collect() had to re-encode on the host (flagged by the device)

    def collect(self, threads: int = 1) -> List[bytes]:
        """Waits for the encode, copies the sizes, offsets and packet bytes (only those) to pinned memory on a stream of its own --
        not behind whatever the caller queued on its streams since -- and returns one packet per frame.  Flagged frames are
        re-encoded on the host (video_io.encode_frame: the same bytes, or its VideoError for a slice of 2^24 bytes or more) and
        counted in host_frames."""
        import torch
        side = torch.cuda.Stream(self.packets.device)
        with torch.cuda.stream(side):
            side.wait_event(self.done)
            h_sizes = torch.empty(self.sizes.shape, dtype=self.sizes.dtype, pin_memory=True)
            h_offsets = torch.empty(self.offsets.shape, dtype=self.offsets.dtype, pin_memory=True)
            h_sizes.copy_(self.sizes, non_blocking=True)
            h_offsets.copy_(self.offsets, non_blocking=True)
            side.synchronize()
            sizes = h_sizes.numpy().view(np.uint32)
            offsets = h_offsets.numpy()
            ok = sizes < TOO_LARGE
            end = int((offsets[ok] + sizes[ok]).max()) if ok.any() else 0
            blob = np.empty(0, np.uint8)
            if end:
                h_blob = torch.empty(end, dtype=torch.uint8, pin_memory=True)
                h_blob.copy_(self.packets[:end], non_blocking=True)
                side.synchronize()
                blob = h_blob.numpy()
            out = []
            for k in range(len(sizes)):
                if ok[k]:
                    o = int(offsets[k])
                    out.append(blob[o:o + int(sizes[k])].tobytes())
                else:
                    self.host_frames += 1
                    out.append(host_packet(self.frames[k], self.slices, self.bgr, threads))
        return out


def host_packet(frame, slices, bgr: bool, threads: int = 1) -> bytes:
    """video_io.encode_frame of one device frame (H, W, 3) or (H, W): the fallback of a flagged frame."""
    from . import video_io
    f = frame.cpu().numpy()
    if f.ndim == 2:
        f = np.repeat(f[..., None], 3, axis=-1)
    return video_io.encode_frame(f, slices=slices, bgr=bgr, threads=threads)[0]


def enqueue(ctx: "_lib.Context", frames, slices=(4, 4), bgr: bool = False, slice_capacity: int = 0,
            packets_cap: Optional[int] = None, stream=None) -> PendingPackets:
    """Enqueues the encode of frames on `stream` (default: the current stream of their device) and returns the buffers it fills."""
    import torch
    N, H, W, ch = check_frames(frames, slices)
    if int(slice_capacity) < 0:
        raise ValueError("slice_capacity must be >= 0 (0 = the default)")
    # the kernel reads rows of W * ch bytes: pixels dense within a row, rows and frames at any pitch
    if frames.stride(2) != ch or (ch == 3 and frames.stride(3) != 1) or frames.stride(1) < W * ch or (N > 1 and frames.stride(0) < frames.stride(1) * H):
        frames = frames.contiguous()
    dev = frames.device
    nh, nv = int(slices[0]), int(slices[1])
    if packets_cap is None:                 # room for every frame at its worst: only a slice past its capacity is flagged
        packets_cap = N * packet_capacity_bytes(W, H, (nh, nv), slice_capacity)
    packets = torch.empty(max(1, int(packets_cap)), dtype=torch.uint8, device=dev)
    offsets = torch.empty(N, dtype=torch.int64, device=dev)
    sizes = torch.empty(N, dtype=torch.int32, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    ctx.check(ctx._L.mdvt_encode_video_frames(ctx.handle, W, H, nh, nv, C.c_void_p(frames.data_ptr()), frames.stride(1),
                                             frames.stride(0), ch, 1 if bgr else 0, N, int(slice_capacity),
                                             C.c_void_p(packets.data_ptr()), int(packets_cap), C.c_void_p(offsets.data_ptr()),
                                             C.c_void_p(sizes.data_ptr()), C.c_void_p(s.cuda_stream)))
    done = torch.cuda.Event()
    done.record(s)
    return PendingPackets(frames, (nh, nv), bgr, packets, offsets, sizes, done)


_contexts = {}


def _context(device: int) -> "_lib.Context":
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = _lib.Context(device, 16, 16)      # (the render size is irrelevant to the encoder)
    return ctx


def encode_frames_on_device(frames, slices=(4, 4), bgr: bool = False, slice_capacity: int = 0,
                            packets_cap: Optional[int] = None) -> List[bytes]:
    """FFV1 packets of (N, H, W, 3) (RGB, or BGR with bgr=True) or (N, H, W) grey uint8 CUDA frames (rows and frames may be
    padded): the same bytes as video_io.encode_frame(frame, slices, bgr) per frame, grey frames as R = G = B.  The defaults
    leave the host nothing to do short of a slice past twice its raw size (enqueue + collect report such frames)."""
    check_frames(frames, slices)
    p = enqueue(_context(frames.device.index if frames.device.index is not None else 0), frames, slices, bgr, slice_capacity,
                packets_cap)
    return p.collect()
