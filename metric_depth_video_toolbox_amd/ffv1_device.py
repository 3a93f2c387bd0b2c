"""FFV1 packets of device frames (mdvt_encode_video_frames): byte for byte those of video_io.encode_frame, without copying the raw
frames to the host.  A frame the device could not code (a slice past its capacity, or a packet past the packet buffer) is
re-encoded on the host, which gives the same bytes, or refuses the frame as the host encoder refuses it.

The other direction (mdvt_decode_video_frames, include/mdvt_ffv1_decode.h): packets of the stream class the project's writer makes
are copied to the device as stored and decoded there into the bytes video_io.VideoReader gives; a frame the device flags is
decoded on the host, which gives the same bytes or the host's own VideoError.

A third part (mdvt_decode_video_stream, include/mdvt_ffv1_stream_decode.h) does the same for streams whose context state carries
from frame to frame: Golomb-Rice or range coder, with inter frames -- the files FFmpeg and OpenCV write by default, RGB or
8-bit YCbCr (yuv444p, yuv422p, yuv420p: converted on the device as include/mdvt_video.h states, the host reader's bytes)."""
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
    """Enqueues the encode of frames on `stream` (default: the current stream of their device) and returns the buffers it fills.
    frames: uint8 [N,H,W,3] or [N,H,W] on the context's GPU; dense pixels with padded rows and frames are read where they lie, any
    other layout (unpacked or transposed pixels, overlapping frames) is encoded from a contiguous copy."""
    import torch
    N, H, W, ch = check_frames(frames, slices)
    if int(slice_capacity) < 0:
        raise ValueError("slice_capacity must be >= 0 (0 = the default)")
    if frames.device.index != ctx.device:
        raise ValueError(f"frames are on {frames.device}, the context on cuda:{ctx.device}")
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
    ctx.call("mdvt_encode_video_frames", W, H, nh, nv, C.c_void_p(frames.data_ptr()), frames.stride(1),
             frames.stride(0), ch, 1 if bgr else 0, N, int(slice_capacity),
             C.c_void_p(packets.data_ptr()), int(packets_cap), C.c_void_p(offsets.data_ptr()),
             C.c_void_p(sizes.data_ptr()), _lib.stream_arg(dev, s))
    done = torch.cuda.Event()
    done.record(s)
    return PendingPackets(frames, (nh, nv), bgr, packets, offsets, sizes, done)


def _context(device) -> "_lib.Context":
    """The shared 16 x 16 context of a GPU (the render size is irrelevant to the codec): _lib.shared_context under the name the
    tests of this module know."""
    return _lib.shared_context(device)


def encode_frames_on_device(frames, slices=(4, 4), bgr: bool = False, slice_capacity: int = 0,
                            packets_cap: Optional[int] = None) -> List[bytes]:
    """FFV1 packets of (N, H, W, 3) (RGB, or BGR with bgr=True) or (N, H, W) grey uint8 CUDA frames (rows and frames may be
    padded): the same bytes as video_io.encode_frame(frame, slices, bgr) per frame, grey frames as R = G = B.  The defaults
    leave the host nothing to do short of a slice past twice its raw size (enqueue + collect report such frames)."""
    check_frames(frames, slices)
    return enqueue(_context(frames.device), frames, slices, bgr, slice_capacity, packets_cap).collect()


# ---------------------------------------------------------------------------------------------------------------------
# decoding
# ---------------------------------------------------------------------------------------------------------------------
DECODE_STATUS = {0: "decoded", 1: "CRC mismatch in a slice", 2: "malformed slice header / rectangle", 3: "bitstream damaged",
                 4: "slice sizes do not add up to the packet"}


def _class_reason(info, config: Optional[bytes], stream: bool) -> Optional[str]:
    """None when the stream of a video_io.VideoInfo (and, when given, its configuration record) is in the intra decoder's class or
    (`stream`) the stream decoder's, else the reason, naming the field."""
    if info.ffv1_version != 3:
        return f"version: FFV1 version {info.ffv1_version} (only version 3 is decoded on the device)"
    if stream and info.coder_type not in (0, 1):
        return f"coder_type {info.coder_type}: a custom state-transition table is not decoded on the device"
    if not stream and info.coder_type != 1:
        return f"coder_type: {info.coder_type} (only the range coder with the default state table, 1, is decoded on the device)"
    if info.alpha:
        return "extra_plane: alpha planes are not decoded on the device"
    if not stream and not info.intra:
        return "intra: only streams whose every frame is a key frame are decoded on the device"
    if not 1 <= info.slices <= 1024:
        return f"num_h_slices / num_v_slices: {info.slices} slices per frame (1 to 1024 are decoded on the device)"
    if config is not None:
        why = _record_reason(config, stream)
        if why:
            return why.decode()
    return None


def _record_reason(config: bytes, stream: bool):
    L = _lib.load()
    return (L.mdvt_ffv1_stream_decode_supported if stream else L.mdvt_ffv1_decode_supported)(config, len(config))


def supported(info, config: Optional[bytes] = None) -> Optional[str]:
    """None when the device decodes the stream of a video_io.VideoInfo (and, when given, its configuration record), else the
    reason, naming the field.  Touches no GPU: the record is parsed by the library's host code."""
    return _class_reason(info, config, False)


def check_out(out, N: int, H: int, W: int) -> None:
    """ValueError unless `out` is a CUDA uint8 tensor of N x H x W x 3 whose pixels are dense (rows and frames may be padded)."""
    import torch
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8:
        raise ValueError("out must be a uint8 torch.Tensor on a CUDA device")
    if tuple(out.shape) != (N, H, W, 3):
        raise ValueError(f"out must be {(N, H, W, 3)}, got {tuple(out.shape)}")
    if out.stride(3) != 1 or out.stride(2) != 3 or out.stride(1) < 3 * W or (N > 1 and out.stride(0) < out.stride(1) * H):
        raise ValueError(f"out must have dense pixels, rows of at least {3 * W} bytes and frames that do not overlap, got strides {out.stride()}")


class PendingFrames:
    """The device side of one decode: `out` (the frames from first_out on) and the status words (one per packet), filled on the
    stream the decode was enqueued on (`done` is recorded there behind it).  The pinned staging buffers live as long as this object."""

    def __init__(self, packets, config, W, H, bgr, out, status, done, staged, first_out=0):
        self.packets, self.config, self.W, self.H, self.bgr, self.first_out = packets, config, W, H, bgr, first_out
        self.out, self.status, self.done, self._staged = out, status, done, staged
        self.host_frames = 0                  # stored frames collect() had to decode on the host (flagged by the device)
        self.flags = None                     # numpy uint32 [packets] after collect(): the device's status words

    def _wait(self) -> None:
        self.done.synchronize()
        self.flags = self.status.cpu().numpy().view(np.uint32)
        self._staged = None

    def collect(self, threads: int = 1):
        """Waits for the decode and reads the status words.  A flagged frame is decoded on the host (video_io.decode_frame: the
        same bytes, or the host's VideoError for a packet the host refuses too), copied into its place and counted in
        host_frames.  -> out"""
        import torch
        from . import video_io
        self._wait()
        for k in np.nonzero(self.flags)[0]:
            self.host_frames += 1
            frame = video_io.decode_frame(self.packets[k], self.config, self.W, self.H, bgr=self.bgr, threads=threads)
            self.out[int(k)].copy_(torch.from_numpy(frame))
        return self.out


class StagedPackets:
    """Packets packed into one pinned blob, with their offsets and sizes (pinned too): what enqueue_decode copies to the device."""

    def __init__(self, packets):
        import torch
        self.packets = list(packets)
        N = len(self.packets)
        if N < 1:
            raise ValueError("no packets")
        sizes = np.array([len(p) for p in self.packets], np.int64)
        if sizes.max() >= 1 << 32:
            raise ValueError("a packet of 4 GiB or more")
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.total = int(sizes.sum())
        self.h_blob = torch.empty(max(1, self.total), dtype=torch.uint8, pin_memory=True)
        blob = self.h_blob.numpy()
        for o, p in zip(offsets, self.packets):
            blob[o:o + len(p)] = np.frombuffer(p, np.uint8)
        self.h_meta = torch.empty(2 * N, dtype=torch.int64, pin_memory=True)
        self.h_meta[:N] = torch.from_numpy(offsets)
        self.h_meta[N:] = torch.from_numpy(sizes)

    def __len__(self):
        return len(self.packets)


def _enqueue_decode(pending, ctx, packets, config, width, height, first_out, bgr, out, stream):
    """Both decoders' staging: the class check, the pinned blob (or a StagedPackets), its copy on a side stream, the call on
    `stream` and the event behind it.  first_out None: mdvt_decode_video_frames, every frame stored; else mdvt_decode_video_stream.
    -> pending(...)"""
    import torch
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError(f"frames of {W} x {H}")
    streamed = first_out is not None
    why = _record_reason(config, streamed)
    if why:
        raise _lib.MdvtError(-3, f"FFV1 stream outside the device {'stream ' if streamed else ''}decoder's class: {why.decode()}")
    staged = packets if isinstance(packets, StagedPackets) else StagedPackets(packets)
    N, total = len(staged), staged.total
    first = int(first_out) if streamed else 0
    if not 0 <= first < N:
        raise ValueError(f"first_out {first} outside [0, {N})")
    dev = torch.device("cuda", ctx.device)
    n_out = N - first
    if out is None:
        out = torch.empty((n_out, H, W, 3), dtype=torch.uint8, device=dev)
    check_out(out, n_out, H, W)
    if out.device.index != ctx.device:
        raise ValueError(f"out is on {out.device}, the context on cuda:{ctx.device}")
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        d_blob = torch.empty(max(1, total), dtype=torch.uint8, device=dev)
        d_meta = torch.empty(2 * N, dtype=torch.int64, device=dev)
        d_blob.copy_(staged.h_blob, non_blocking=True)
        d_meta.copy_(staged.h_meta, non_blocking=True)
        d_sizes = d_meta[N:].to(torch.int32)
        status = torch.empty(N, dtype=torch.int32, device=dev)
        copied = torch.cuda.Event()
        copied.record(side)
    s.wait_event(copied)
    for t in (d_blob, d_meta, d_sizes, status):
        t.record_stream(s)
    ctx.call("mdvt_decode_video_stream" if streamed else "mdvt_decode_video_frames", W, H, config, len(config),
             C.c_void_p(d_blob.data_ptr()), total, C.c_void_p(d_meta.data_ptr()), C.c_void_p(d_sizes.data_ptr()), N,
             *((first,) if streamed else ()),
             C.c_void_p(out.data_ptr()), out.stride(1), out.stride(0) if n_out > 1 else out.stride(1) * H,
             1 if bgr else 0, C.c_void_p(status.data_ptr()), _lib.stream_arg(dev, s))
    done = torch.cuda.Event()
    done.record(s)
    return pending(staged.packets, config, W, H, bgr, out, status, done, (staged, d_blob, d_meta, d_sizes), first)


def enqueue_decode(ctx: "_lib.Context", packets, config: bytes, width: int, height: int, bgr: bool = False, out=None,
                   stream=None) -> PendingFrames:
    """Packs the packets into one pinned blob (or takes a StagedPackets), copies it on a side stream and enqueues the decode into
    `out` (default: a new N x H x W x 3 tensor on the ctx's device) on `stream` (default: the current stream).  MdvtError
    (MDVT_ERR_UNSUPPORTED) for a configuration record outside the device's class, before anything is copied."""
    return _enqueue_decode(PendingFrames, ctx, packets, config, width, height, None, bgr, out, stream)


def decode_frames_on_device(packets, config: bytes, width: int, height: int, *, bgr: bool = False, out=None, stream=None,
                            device: int = 0):
    """-> (frames, status): the N x H x W x 3 uint8 CUDA frames video_io.VideoReader gives for these packets (RGB, or BGR with
    bgr=True; into `out`, whose rows and frames may be padded) and the device's status words (numpy uint32 [N]; a nonzero word:
    that frame was decoded on the host instead)."""
    p = enqueue_decode(_context(device if out is None else out.device), packets, config, width, height, bgr, out, stream)
    frames = p.collect()
    return frames, p.flags


# ---------------------------------------------------------------------------------------------------------------------
# decoding streams whose context state carries from frame to frame (mdvt_decode_video_stream, include/mdvt_ffv1_stream_decode.h)
# ---------------------------------------------------------------------------------------------------------------------
NO_KEY_FRAME, BROKEN_RUN = 5, 6
STREAM_STATUS = {**DECODE_STATUS, NO_KEY_FRAME: "no key frame at or before this frame inside the call",
                 BROKEN_RUN: "an earlier frame of this key-frame run was flagged"}


def stream_supported(info, config: Optional[bytes] = None) -> Optional[str]:
    """supported() for the stream decoder's class: version 3, coder_type 0 or 1, intra 0 or 1, RGB or YCbCr in 4:4:4, 4:2:2, 4:2:0
    (the files FFmpeg and OpenCV write by default are in it).  None, or the reason, naming the field."""
    return _class_reason(info, config, True)


def packet_is_key(packet: bytes) -> bool:
    """The packet's key-frame bit (mdvt_ffv1_packet_is_key: its first range-coded bit); a packet too short to have one is none."""
    return _lib.load().mdvt_ffv1_packet_is_key(packet, len(packet)) == 1


class PendingStreamFrames(PendingFrames):
    """The device side of one stream decode: `out` holds frames first_out ... of the packets, `status` one word per packet."""

    def collect(self, threads: int = 1):
        """Waits for the decode and reads the status words.  A flagged frame cannot be decoded alone: the host decodes its whole
        key-frame run from the run's key frame (video_io.StreamDecoder: the same bytes, or the host's VideoError), and every stored
        frame of the run from the first flagged one on is copied into its place and counted in host_frames.  -> out"""
        import torch
        from . import video_io
        self._wait()
        bad = np.nonzero(self.flags[self.first_out:])[0] + self.first_out
        done_to = -1
        for k in bad:
            k = int(k)
            if k <= done_to:
                continue
            start = k
            while start > 0 and not packet_is_key(self.packets[start]):
                start -= 1
            if not packet_is_key(self.packets[start]):
                raise video_io.VideoError(f"FFV1: frame {k} of the call has no key frame at or before it")
            end = k + 1
            while end < len(self.packets) and not packet_is_key(self.packets[end]):
                end += 1
            with video_io.StreamDecoder(self.config, self.W, self.H, bgr=self.bgr, threads=threads) as dec:
                for j in range(start, end):
                    frame = dec.decode(self.packets[j])
                    if j >= k and j >= self.first_out:
                        self.host_frames += 1
                        self.out[j - self.first_out].copy_(torch.from_numpy(frame))
            done_to = end - 1
        return self.out


def enqueue_decode_stream(ctx: "_lib.Context", packets, config: bytes, width: int, height: int, first_out: int = 0, bgr: bool = False,
                          out=None, stream=None) -> PendingStreamFrames:
    """enqueue_decode for consecutive packets of one stream of the stream decoder's class.  Frames first_out ... are stored in `out`
    (default: a new (N - first_out) x H x W x 3 tensor); the packets before first_out are decoded for their context state alone
    (the caller prepends them from the last key frame on).  State is not carried from one call to the next."""
    return _enqueue_decode(PendingStreamFrames, ctx, packets, config, width, height, int(first_out), bgr, out, stream)


def decode_stream_on_device(packets, config: bytes, width: int, height: int, *, first_out: int = 0, bgr: bool = False, out=None,
                            stream=None, device: int = 0):
    """-> (frames, status, host_frames): frames first_out ... of consecutive packets as video_io.VideoReader gives them, the
    device's status words (numpy uint32, one per packet) and the count of stored frames the host had to decode instead."""
    p = enqueue_decode_stream(_context(device if out is None else out.device), packets, config, width, height, first_out, bgr, out, stream)
    frames = p.collect()
    return frames, p.flags, p.host_frames
