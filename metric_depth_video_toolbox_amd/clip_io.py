"""The file side of a clip: the frame files the drivers read and write (FFV1-in-Matroska videos through video_io, `.npy` frame
dumps, per-rank segments + index), the tmp -> final protocol (dfh:163-179), and the plumbing the clip scripts share around their
batch loops (basic_nomal_infill, stereo_crafter_infill, find_convergence_depth, video_metric_convert): open_frames / fetch,
ClipInputs and ClipOutput.  Imports neither the renderer nor torch at module level, so every script can import it at its top."""
from __future__ import annotations

import json
import os
import threading
from typing import Optional

import numpy as np

from . import _lib, video_io


class _RawFrames:
    """Frame dumps that live in a file (np.load(..., mmap_mode=...) / open_memmap arrays) are read and written with
    pread / pwrite straight between the file and the pinned staging buffers: one kernel copy per batch and direction,
    no page-fault storm through a mapping and no intermediate NumPy array.  Anything else (plain arrays, lists) is
    indexed the ordinary way."""

    def __init__(self, arr, writable: bool):
        self.arr = arr
        self.fd = -1
        if isinstance(arr, (VideoFrames, VideoSink)):           # a video file: its own decode / encode-and-append
            self.read_into = arr.read_into if isinstance(arr, VideoFrames) else None
            self.write_from = arr.write_from if isinstance(arr, VideoSink) else None
            return
        if isinstance(arr, np.memmap) and arr.flags["C_CONTIGUOUS"] and getattr(arr, "filename", None) and arr.ndim >= 2:
            # A slice of a memmap (depth[k:]) is still an np.memmap with the parent's filename AND the parent's `offset`:
            # the file position of its first byte is the root mapping's offset plus the distance of the data pointers.
            root = arr
            while isinstance(getattr(root, "base", None), np.memmap):
                root = root.base
            try:
                delta = int(arr.__array_interface__["data"][0]) - int(root.__array_interface__["data"][0])
                if delta < 0 or len(arr) == 0:
                    raise OSError("not a forward slice of its mapping")
                self.fd = os.open(str(arr.filename), os.O_RDWR if writable else os.O_RDONLY)
                self.base = int(root.offset) + delta
                self.frame_bytes = int(arr[0].nbytes)
            except (OSError, KeyError, TypeError):
                self.fd = -1

    def read_into(self, dst: np.ndarray, a: int, n: int):
        if self.fd < 0:
            dst[...] = self.arr[a:a + n]
            return
        mv = memoryview(dst).cast("B")
        off, done, total = self.base + a * self.frame_bytes, 0, n * self.frame_bytes
        while done < total:
            got = os.preadv(self.fd, [mv[done:total]], off + done)
            if got <= 0:
                raise IOError("short read from a frame dump")
            done += got

    def write_from(self, src: np.ndarray, a: int, n: int):
        if self.fd < 0:
            self.arr[a:a + n] = src
            return
        mv = memoryview(src).cast("B")
        off, done, total = self.base + a * self.frame_bytes, 0, n * self.frame_bytes
        while done < total:
            done += os.pwritev(self.fd, [mv[done:total]], off + done)

    def close(self):
        if self.fd >= 0:
            os.close(self.fd)
            self.fd = -1


class VideoFrames:
    """An FFV1-in-Matroska file as the read-only [N, H, W, 3] uint8 frame array render_clip / open_output expect (RGB order).
    Reads go through a small pool of decoders: a sequential reader continues where its decoder stands, anything else is a
    seek (free in an intra-only stream; an inter-coded one -- FFmpeg's default, a key frame every 12 -- decodes forward from the
    last key frame, so it gets ONE decoder and all the slice threads instead of several decoders leap-frogging)."""

    def __init__(self, path: str, readers: int = 2, threads: Optional[int] = None):
        """threads: slice threads per reader (default: the usable cores shared among the readers; an inter-coded file's one reader
        gets one per slice, capped at the cores)."""
        from . import video_io
        first = video_io.VideoReader(path)
        self.path, self.fps, self.info = path, first.fps, first.info
        self.pix_fmt = first.pix_fmt                         # what the stream codes; the frames are RGB either way
        self.shape = (first.frames, first.height, first.width, 3)
        self.dtype, self.ndim = np.dtype(np.uint8), 4
        n = max(1, int(readers)) if first.info.intra else 1
        cores = _usable_cores()
        first.threads = int(threads) if threads is not None else max(1, cores // (2 * n)) if n > 1 else 0
        self._readers = [first] + [video_io.VideoReader(path, threads=first.threads) for _ in range(n - 1)]
        self._pos = [0] * n
        self._busy = [False] * n
        self._cv = threading.Condition()
        # render_clip decodes this file's frames on the device (use_device_decoder): it asks for packets, not for frames
        self.device_decode = False
        # ... with mdvt_decode_video_stream (inter-coded / Golomb-Rice files, video_decoder "device_all"): read_stream_packets
        self.stream_decode = False
        self._packet_reader = None

    def __len__(self):
        return self.shape[0]

    def use_device_decoder(self, name: str = "input", video_decoder: str = "device") -> bool:
        """Switches render_clip's reads of this file to the device decoder (ffv1_device) if the stream is in its class; if not,
        says so on stderr and leaves the host decoder in charge (files the reference made must keep working).  "device_all" also
        takes the stream decoder's class (Golomb-Rice, inter frames: what FFmpeg and OpenCV write by default) to the device."""
        import sys
        from . import ffv1_device
        self.config = self._readers[0].config_record()
        self.decoder_name = name
        why = ffv1_device.supported(self.info, self.config)
        if why is not None and video_decoder == "device_all":
            why = ffv1_device.stream_supported(self.info, self.config)
            self.stream_decode = why is None
        if why is not None:
            print(f"video_decoder {video_decoder}: {name} {self.path} is decoded on the host ({why})", file=sys.stderr)
            return False
        self.device_decode = True
        return True

    def read_stream_packets(self, a: int, n: int):
        """For a file of the stream decoder's class: (the packets from the last key frame at or before frame a up to frame
        a + n - 1, the index of frame a among them = mdvt_decode_video_stream's first_out).  The key frame is looked for at most
        KEY_SCAN_FRAMES frames back (two bytes read per frame: VideoReader.packet_is_key); None when there is none that near: the
        caller gives the file to the host reader (host_after_far_key_frame)."""
        self.read_packets(a, 0)                              # (makes the packet reader)
        r = self._packet_reader
        lo = max(0, a - KEY_SCAN_FRAMES)
        k = a
        with r[2]:
            while not r[0].packet_is_key(k):
                if k == lo:
                    return None
                k -= 1
        return self.read_packets(k, a - k + n), a - k

    def host_after_far_key_frame(self):
        """Hands a file whose key frames lie further apart than KEY_SCAN_FRAMES back to the host decoder, with one stderr line."""
        import sys
        if self.device_decode:
            self.device_decode = self.stream_decode = False
            print(f"video_decoder device_all: {self.decoder_name} {self.path} is decoded on the host (intra: a key-frame distance of more "
                  f"than {KEY_SCAN_FRAMES} frames; the device decodes a call's frames from the key frame before them)", file=sys.stderr)

    def read_packets(self, a: int, n: int):
        """The stored FFV1 packets of frames a ... a + n - 1 (a reader of its own: packets are not decoded, so nothing is shared
        with the decoders' positions)."""
        with self._cv:
            if self._packet_reader is None:
                from . import video_io
                self._packet_reader = [video_io.VideoReader(self.path, threads=1), -1, threading.Lock()]
        r = self._packet_reader
        with r[2]:
            if r[1] != a:
                r[0].seek_packet(a) if self.stream_decode else r[0].seek(a)
            out = []
            for i in range(n):
                pkt = r[0].next_packet()
                if pkt is None:
                    r[1] = -1
                    raise IOError(f"{self.path}: ends at frame {a + i}")
                out.append(pkt)
            r[1] = a + n
        return out

    def read_into(self, dst: np.ndarray, a: int, n: int):
        with self._cv:
            while True:
                free = [k for k in range(len(self._readers)) if not self._busy[k]]
                if free:
                    k = next((k for k in free if self._pos[k] == a), None)
                    if k is None:
                        behind = [k for k in free if self._pos[k] <= a]
                        k = max(behind, key=lambda q: self._pos[q]) if behind else free[0]
                    self._busy[k] = True
                    break
                self._cv.wait()
        try:
            r = self._readers[k]
            if self._pos[k] != a:
                r.seek(a)
            for i in range(n):
                if not r.read_into(dst[i]):
                    raise IOError(f"{self.path}: ends at frame {a + i}")
            self._pos[k] = a + n
        except BaseException:
            self._pos[k] = -1 << 60         # unknown position: the next use seeks
            raise
        finally:
            with self._cv:
                self._busy[k] = False
                self._cv.notify()

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            lo, hi, step = idx.indices(len(self))
            if step != 1:
                return np.stack([self[t] for t in range(lo, hi, step)]) if hi > lo else np.empty((0,) + self.shape[1:], np.uint8)
            out = np.empty((max(0, hi - lo),) + self.shape[1:], np.uint8)
            if hi > lo:
                self.read_into(out, lo, hi - lo)
            return out
        t = int(idx)
        if t < 0:
            t += len(self)
        out = np.empty((1,) + self.shape[1:], np.uint8)
        self.read_into(out, t, 1)
        return out[0]

    def __array__(self, dtype=None, copy=None):
        a = self[0:len(self)]
        return a if dtype is None else a.astype(dtype)

    def close(self):
        for r in self._readers:
            r.close()
        if self._packet_reader is not None:
            self._packet_reader[0].close()


VIDEO_ENCODERS = ("host", "device")


# "device": the class this project's writer makes goes to the device (mdvt_decode_video_frames).  "device_all": that, and the
# stream decoder's class as well (mdvt_decode_video_stream: Golomb-Rice or range coder with inter frames, RGB or YCbCr -- a colour
# video FFmpeg coded as yuv420p is in it, and outside "device"'s class like any other file of FFmpeg's).  Anything else: the host.
VIDEO_DECODERS = ("host", "device", "device_all")

# How far back fetch() looks for the key frame in front of a batch of a "device_all" file: FFmpeg's default distance is 12, twice
# that must work; 64 keeps the frames decoded for their state alone below the size of a usual batch of 64.  State is not carried
# from one fetch to the next, so every batch pays for the frames between its key frame and its first frame.
KEY_SCAN_FRAMES = 64


class VideoSink:
    """An output video being written: render_clip's store threads hand it frame sub-ranges in any order (write_from), each
    thread encodes its frames itself (one FFV1 packet per frame, slices on one thread: the parallelism is across frames) and
    the packets are appended in frame order.  Grey frames (the hole mask) are written as R = G = B.
    encoder="device": render_clip enqueues the encode of each batch on the device right after the frames are made (enqueue:
    mdvt_encode_video_frames, the same bytes) and its store stage appends the packets (append_packets); only the packet bytes
    leave the device.  write_from stays available in both modes (host encode)."""

    def __init__(self, path: str, width: int, height: int, fps: float, grey: bool = False, slices=(4, 4), bgr: bool = False,
                 encoder: str = "host"):
        import threading
        from . import video_io
        if encoder not in VIDEO_ENCODERS:
            raise ValueError(f"encoder must be one of {VIDEO_ENCODERS}, got {encoder!r}")
        self._vio, self.bgr, self.device = video_io, bgr, encoder == "device"
        self.slices = (min(slices[0], width), min(slices[1], height))
        self._w = video_io.VideoWriter(path, width, height, fps, slices=self.slices)
        self.path, self.grey, self.shape_hw = path, grey, (height, width)
        self._pending, self._next, self._lock = {}, 0, threading.Lock()
        self.host_frames = 0             # device mode: frames the device flagged, re-encoded on the host (reported by close)

    def _append(self, t: int, pkt: bytes):
        with self._lock:
            self._pending[t] = pkt
            while self._next in self._pending:
                self._w.write_packet(self._pending.pop(self._next))
                self._next += 1

    def write_from(self, src: np.ndarray, a: int, n: int):
        for i in range(n):
            f = src[i]
            if self.grey:
                f = np.repeat(f[..., None], 3, axis=-1)
            pkt, _ = self._vio.encode_frame(f, slices=self.slices, threads=1, bgr=self.bgr)
            self._append(a + i, pkt)

    def enqueue(self, ctx, frames):
        """Enqueues the device encode of frames ([n, H, W, 3] or grey [n, H, W] on the current stream) -> ffv1_device.PendingPackets."""
        from . import ffv1_device
        return ffv1_device.enqueue(ctx, frames, slices=self.slices, bgr=self.bgr)

    def append_packets(self, pending, a: int):
        """The packets of an enqueue()d batch (its stream work done), as frames a, a + 1, ...  Frames the device flagged are
        encoded on the host."""
        for i, pkt in enumerate(pending.collect()):
            self._append(a + i, pkt)
        if pending.host_frames:
            with self._lock:
                self.host_frames += pending.host_frames

    def close(self) -> int:
        with self._lock:
            if self._pending:
                missing = self._next
                self._pending.clear()
                self._w.close()
                raise RuntimeError(f"{self.path}: frame {missing} was never written")
            if self.host_frames:
                import warnings
                warnings.warn(f"{self.path}: {self.host_frames} frame(s) had a slice past its device capacity and were encoded on "
                              "the host (same bytes)")
            return self._w.close()


def npy_shape(path: str):
    """Shape recorded in a .npy header (no mapping: an empty segment cannot be mapped)."""
    with open(path, "rb") as fh:
        major, _ = np.lib.format.read_magic(fh)
        shape, _, _ = (np.lib.format.read_array_header_1_0 if major == 1 else np.lib.format.read_array_header_2_0)(fh)
    return shape


def frames_in(path: str) -> int:
    """Frames in an output file of either kind (a .npy header, or the frames indexed in a Matroska file: what the reference asks
    cv2.CAP_PROP_FRAME_COUNT for, dfh:169)."""
    from . import video_io
    if video_io.is_matroska(path):
        with video_io.VideoReader(path) as r:
            return r.frames
    return npy_shape(path)[0]


def verify_and_move(tmp_path: str, expected_frames: int, final_path: str):
    """The reference's tmp -> final protocol (dfh:163-179): rename only if the frame count matches."""
    got = frames_in(tmp_path)
    if got != expected_frames:
        raise RuntimeError(f"{tmp_path}: {got} frames written, expected {expected_frames}; left in place")
    os.replace(tmp_path, final_path)


def segment_path(path: str, rank: int, world: int) -> str:
    """File of rank `rank`'s output segment: `<path>` itself for a single rank, else `<path>.rank<r>of<R><ext of path>`."""
    return path if world == 1 else f"{path}.rank{rank}of{world}{os.path.splitext(path)[1] or '.npy'}"


class SegmentedFrames:
    """Read-only view of an output written as per-rank segments: indexable like the single [N, ...] array."""

    def __init__(self, parts, bounds):
        self.parts, self.bounds = parts, bounds          # bounds[k] = first frame of part k; bounds[-1] = N
        self.shape = (bounds[-1],) + tuple(parts[0].shape[1:])
        self.dtype = parts[0].dtype
        self.ndim = len(self.shape)

    def __len__(self):
        return self.bounds[-1]

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            lo, hi, step = idx.indices(len(self))
            if step != 1:
                return np.stack([self[t] for t in range(lo, hi, step)])
            out = [p[max(lo, b0) - b0:min(hi, b1) - b0] for p, b0, b1 in zip(self.parts, self.bounds[:-1], self.bounds[1:])
                   if max(lo, b0) < min(hi, b1)]
            return np.concatenate(out) if out else np.empty((0,) + self.shape[1:], self.dtype)
        t = int(idx)
        if t < 0:
            t += len(self)
        k = int(np.searchsorted(self.bounds, t, side="right")) - 1
        return self.parts[k][t - self.bounds[k]]

    def __array__(self, dtype=None, copy=None):
        a = self[0:len(self)]
        return a if dtype is None else a.astype(dtype)


def open_output(path: str, mmap_mode: Optional[str] = "r"):
    """An output of run(): the single dump `<path>` or the per-rank segments named by `<path>.index.json` (run() leaves only the
    form it wrote; should both exist -- files copied together by hand -- the newer one is taken)."""
    from . import video_io

    def one(f, mapped=True):
        return VideoFrames(f, readers=1) if video_io.is_matroska(f) else np.load(f, mmap_mode=mmap_mode if mapped else None)
    ip = path + ".index.json"
    if os.path.exists(path) and not (os.path.exists(ip) and os.path.getmtime(ip) > os.path.getmtime(path)):
        return one(path)
    with open(path + ".index.json") as fh:
        idx = json.load(fh)
    here = os.path.dirname(path)
    parts = [one(os.path.join(here, s["file"]), s["hi"] > s["lo"]) for s in idx["segments"]]
    bounds = [s["lo"] for s in idx["segments"]] + [idx["frames"]]
    for p, s in zip(parts, idx["segments"]):
        if p.shape[0] != s["hi"] - s["lo"]:
            raise RuntimeError(f"{s['file']}: {p.shape[0]} frames, the index says {s['hi'] - s['lo']}")
    return SegmentedFrames(parts, bounds)


def _remove_segments(path: str, keep=()):
    """Remove `<path>.index.json` and the segment files it names (an earlier multi-rank run's form of the output), except the
    files named in `keep` (base names: the segments the run that calls this has just written)."""
    ip = path + ".index.json"
    if not os.path.exists(ip):
        return
    try:
        with open(ip) as fh:
            idx = json.load(fh)
        for s in idx.get("segments", []):
            if s["file"] in keep:
                continue
            f = os.path.join(os.path.dirname(path), s["file"])
            if os.path.exists(f):
                os.remove(f)
    finally:
        os.remove(ip)


def merge_output(path: str, remove_segments: bool = True) -> str:
    """Concatenate the segments of `<path>.index.json` into the single dump `<path>` (tmp -> final rename)."""
    seg = open_output(path)
    if not isinstance(seg, SegmentedFrames):
        return path
    if isinstance(seg.parts[0], VideoFrames):
        # video segments: the packets are copied as they are (every segment was written with the same size and slice counts)
        from . import video_io
        tmp = path + ".merge_tmp.mkv"
        first = video_io.VideoReader(seg.parts[0].path)
        H, W = first.height, first.width
        sl = (min(4, W), min(4, H))                    # VideoSink's slice grid
        if first.info.slices != sl[0] * sl[1]:
            raise RuntimeError(f"{seg.parts[0].path}: {first.info.slices} slices per frame, not one of this driver's segments")
        first.close()
        with video_io.VideoWriter(tmp, W, H, seg.parts[0].fps, slices=sl) as w:
            for part in seg.parts:
                with video_io.VideoReader(part.path) as r:
                    while True:
                        pkt = r.next_packet()
                        if pkt is None:
                            break
                        w.write_packet(pkt)
        for part in seg.parts:
            part.close()
    else:
        tmp = path + ".merge_tmp.npy"
        out = np.lib.format.open_memmap(tmp, mode="w+", dtype=seg.dtype, shape=seg.shape)
        for p, b0 in zip(seg.parts, seg.bounds[:-1]):
            out[b0:b0 + p.shape[0]] = p
        out.flush()
        del out
    os.replace(tmp, path)
    if remove_segments:
        with open(path + ".index.json") as fh:
            idx = json.load(fh)
        for s in idx["segments"]:
            os.remove(os.path.join(os.path.dirname(path), s["file"]))
        os.remove(path + ".index.json")
    return path


def _usable_cores() -> int:
    """Cores this process may use: affinity mask capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = max(1, min(n, int(float(q) / float(per))))
    except Exception:
        pass
    return n


def check_video_encoder(video_encoder: str, video: bool):
    """ValueError unless video_encoder is "host" or "device", and "device" only where the outputs are .mkv files."""
    if video_encoder not in VIDEO_ENCODERS:
        raise ValueError(f"video_encoder must be one of {VIDEO_ENCODERS}, got {video_encoder!r}")
    if video_encoder == "device" and not video:
        raise ValueError("--video_encoder device encodes .mkv outputs: with a .npy depth input the outputs are raw .npy dumps, "
                         "which are not encoded (use the default --video_encoder host)")


def check_video_decoder(video_decoder: str, video: bool) -> str:
    """ValueError unless video_decoder is one of VIDEO_DECODERS, and a device decoder only where the inputs are .mkv files."""
    if video_decoder not in VIDEO_DECODERS:
        raise ValueError(f"video_decoder must be one of {VIDEO_DECODERS}, got {video_decoder!r}")
    if video_decoder != "host" and not video:
        raise ValueError(f"--video_decoder {video_decoder} decodes .mkv inputs: a .npy input is a raw frame dump, which is not decoded "
                         "(use the default --video_decoder host)")
    return video_decoder


# ---------------------------------------------------------------------------------------------------------------------
# what the clip scripts share around their batch loops
# ---------------------------------------------------------------------------------------------------------------------
def open_frames(path: str, missing: Exception, run_output: bool = False):
    """A clip as a read-only [N, ...] frame array: `.mkv` -> VideoFrames, `.npy` -> a memmap; run_output: the file is an output of
    clip.run, which may also exist as per-rank segments named by `<path>.index.json` (open_output).  Raises `missing` -- the
    calling script's own exception -- when there is no such file."""
    if not (os.path.isfile(path) or (run_output and os.path.isfile(path + ".index.json"))):
        raise missing
    if run_output:
        return open_output(path)
    return VideoFrames(path) if video_io.is_matroska(path) else np.load(path, mmap_mode="r")


def video_parts(frames):
    """[(VideoFrames, first frame)] of opened frames that are one video or per-rank video segments; [] for frame dumps."""
    if isinstance(frames, VideoFrames):
        return [(frames, 0)]
    if isinstance(frames, SegmentedFrames) and all(isinstance(p, VideoFrames) for p in frames.parts):
        return list(zip(frames.parts, frames.bounds[:-1]))
    return []


def fetch(frames, a: int, b: int, dev, dec_ctx):
    """Frames [a, b) as a uint8 CUDA tensor.  Videos switched to the device decoder hand over their packets (decoded on the
    device, straight into the tensor); everything else is read on the host and copied."""
    import torch
    parts = video_parts(frames)
    if dec_ctx is None or not parts or not all(p.device_decode for p, _ in parts):
        return torch.from_numpy(np.array(frames[a:b])).to(dev)
    from . import ffv1_device
    H, W = int(frames.shape[1]), int(frames.shape[2])
    out = torch.empty((b - a, H, W, 3), dtype=torch.uint8, device=dev)
    for p, b0 in parts:
        lo, hi = max(a, b0), min(b, b0 + len(p))
        if lo >= hi:
            continue
        if not p.stream_decode:
            ffv1_device.enqueue_decode(dec_ctx, p.read_packets(lo - b0, hi - lo), p.config, W, H, out=out[lo - a:hi - a]).collect()
            continue
        got = p.read_stream_packets(lo - b0, hi - lo)
        if got is None:                                      # key frames too far apart: this file is the host's from here on
            p.host_after_far_key_frame()
            return torch.from_numpy(np.array(frames[a:b])).to(dev)
        ffv1_device.enqueue_decode_stream(dec_ctx, got[0], p.config, W, H, first_out=got[1], out=out[lo - a:hi - a]).collect()
    return out


class ClipInputs:
    """The opened inputs of a clip script.  `open` adds a file (open_frames; `name` is what the device decoder's stderr line calls
    it), `on_device` picks the GPU, `fetch` reads a batch.  Leaving the block, normally or by an exception, closes the context and
    every reader: the checks on what was opened belong inside the block."""

    def __init__(self):
        self.opened, self.dev, self.ctx, self.dec_ctx = [], None, None, None

    def __enter__(self):
        return self

    def open(self, path: str, name: str, missing: Exception, run_output: bool = False):
        frames = open_frames(path, missing, run_output)
        self.opened.append((name, frames))
        return frames

    def on_device(self, dev, video_decoder: str = "host", video_encoder: str = "host", *, own_context: bool = False):
        """Reads go to `dev` from here on.  With a "device" codec -- or own_context, for a script whose own calls need one whatever
        the codecs -- this makes the context the decoder and the encoder run in (its own workspace; the render size does not
        matter to them); video_decoder "device" / "device_all" switches every video part over whose stream is in that decoder's class."""
        self.dev = dev
        if own_context or video_decoder in ("device", "device_all") or video_encoder == "device":
            self.ctx = _lib.Context(dev.index, 16, 16)
        if video_decoder in ("device", "device_all"):
            self.dec_ctx = self.ctx
            for name, frames in self.opened:
                for p, _ in video_parts(frames):
                    p.use_device_decoder(name, video_decoder)

    def fetch(self, frames, a: int, b: int):
        return fetch(frames, a, b, self.dev, self.dec_ctx)

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.close()
        for _, frames in self.opened:
            for p, _ in video_parts(frames):
                p.close()


class ClipOutput:
    """An output clip of n uint8 frames being written as `tmp`: a `.npy` dump (fps None), or a video at `fps` coded by the host or
    -- encoder "device", in `ctx` -- on the GPU.  A normal exit from the block closes the file and renames it to `final` if its
    frame count is right (verify_and_move); an exception closes it, removes it and goes on propagating."""

    def __init__(self, tmp: str, final: str, n: int, frame_shape, fps: Optional[float] = None, encoder: str = "host", ctx=None):
        self.tmp, self.final, self.n, self.ctx = tmp, final, int(n), ctx
        self.sink = self.arr = None
        if fps is not None:
            self.sink = VideoSink(tmp, int(frame_shape[1]), int(frame_shape[0]), fps, encoder=encoder)
        else:
            self.arr = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.uint8, shape=(self.n,) + tuple(frame_shape))

    def __enter__(self):
        return self

    def store(self, d_frames, a: int):
        """Frames a, a + 1, ... of the output from a uint8 CUDA tensor."""
        if self.sink is None:
            self.arr[a:a + len(d_frames)] = d_frames.cpu().numpy()
        elif self.sink.device:
            self.sink.append_packets(self.sink.enqueue(self.ctx, d_frames), a)
        else:
            self.sink.write_from(d_frames.cpu().numpy(), a, len(d_frames))

    def __exit__(self, failed, *exc):
        try:
            if self.sink is not None:
                self.sink.close()
            else:
                self.arr.flush()
        except Exception:
            if failed is None:                               # the close itself is what failed
                self._remove()
                raise
        if failed is None:
            self.arr = None
            verify_and_move(self.tmp, self.n, self.final)
        else:
            self._remove()                                   # no half-written tmp file stays; the first error goes on propagating

    def _remove(self):
        self.arr = None
        if os.path.exists(self.tmp):
            os.remove(self.tmp)
