"""What the model-step tools (tools/video_da3.py, depth_engine_video.py, upscale_depth_promptda.py, generate_video_mask.py and
video_mvsa.py) share one level above clip_io's frame I/O, as infill_clip.py does for the infill scripts: the host helpers their host
modules export, the clip session in its two phases, the list loop, and the argument helpers of the tools' device wrappers.  A tool
configures these with what is its own: the exception of a missing file, the rule for the frame count, the frame rate of a file that
states none, the banner.  No tensor's address is taken here: the device wrappers are step_device.py's.
"""
from __future__ import annotations

import json
from contextlib import contextmanager

import numpy as np

from .clip_io import VIDEO_DECODERS, VIDEO_ENCODERS, ClipInputs, ClipOutput, check_video_decoder, check_video_encoder, video_parts
from .infill_clip import callable_from_spec, is_txt, read_list_file      # noqa: F401 (the host modules take callable_from_spec from here)


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------

def clips_from_argument(color_video: str):
    """The clip, or the entries of a .txt list (vd3:301-307, gvm:47-62, 150-155)."""
    return read_list_file(color_video) if is_txt(color_video) else [color_video]


def frames_to_write(n_in_file: int, max_frames: int) -> int:
    """How many frames a per-frame script's loop writes (u3d:155-163, mge:149-157, dpr:134-142, pda:43-58, gvm:85-109): all of them
    with -1, else the first max_frames; the loops test max_frames against the count after counting the frame, so N gives exactly N
    and 0 gives none."""
    n = int(n_in_file)
    return n if int(max_frames) == -1 else max(0, min(n, int(max_frames)))


def output_pair(path: str, video: bool = True, what: str = "depth"):
    """(tmp, final) = (`<path>_tmp_<what>.<ext>`, `<path>_<what>.<ext>`); a .npy frame dump gives a .npy dump."""
    ext = ".mkv" if video else ".npy"
    return path + "_tmp_" + what + ext, path + "_" + what + ext


def write_float_list(path: str, values):
    with open(path, "w") as fh:
        fh.write(json.dumps([float(v) for v in values]))


def add_device_flags(p, batch=None, batch_help=None):
    """The flags that are not the reference's: --batch where the tool has one (its default and what a batch is), --video_decoder and
    --video_encoder."""
    if batch is not None:
        p.add_argument("--batch", default=batch, type=int, help="not a reference flag: " + batch_help)
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="not a reference flag: where an .mkv input is FFV1-decoded -- 'host' (default), 'device' or 'device_all'")
    p.add_argument("--video_encoder", choices=VIDEO_ENCODERS, default="host",
                   help="not a reference flag: where the .mkv output is FFV1-encoded -- 'host' (default) or 'device' (the same bytes)")
    return p


# ---- the clip session ---------------------------------------------------------------------------------------------------------------

class StepClip(ClipInputs):
    """One clip of a model step, in two phases inside one `with StepClip() as clip:` block.  open_checked is the host phase: it
    touches no GPU and makes no context, and neither does the tool's own host work that follows it (a schedule, intrinsics, the
    output names), so a refusal there writes nothing.  device(tmp, final) is the device phase.  Leaving the outer block closes the
    context and every reader (ClipInputs)."""

    def open_checked(self, inputs, video_decoder: str, video_encoder: str, count, default_fps: float = 30.0, label: str = "{path}"):
        """inputs: [(path, argument name, the tool's own exception where there is no such file)], the colour video first.
        count(frames of the shortest input) -> how many are processed.  label: what the shape message calls an input.
        -> the opened inputs; video, H, W, n and fps (the colour video's, default_fps where its file states none, None for frame
        dumps) are this object's from here on."""
        frames = [self.open(path, name, missing) for path, name, missing in inputs]
        self.video = bool(video_parts(frames[0]))
        if any(bool(video_parts(f)) != self.video for f in frames[1:]):
            raise ValueError(" and ".join(f"--{name}" for _, name, _ in inputs) + " must both be .mkv videos or both .npy frame dumps")
        check_video_decoder(video_decoder, self.video)
        check_video_encoder(video_encoder, self.video)
        for (path, name, _), f in zip(inputs, frames):
            if f.ndim != 4 or f.shape[-1] != 3 or f.dtype != np.uint8:
                raise ValueError(label.format(path=path, name=name) + ": uint8 [N, H, W, 3] expected")
        self.H, self.W = int(frames[0].shape[1]), int(frames[0].shape[2])
        self.n = int(count(min(int(f.shape[0]) for f in frames)))
        if self.n < 1:
            raise ValueError("No frames read")                      # dfh:278, mvs:99
        self.fps = (video_parts(frames[0])[0][0].fps or default_fps) if self.video else None
        self.codecs = (video_decoder, video_encoder)
        return frames

    @contextmanager
    def device(self, tmp: str, final: str):
        """The current device, the decoders switched over, ONE context for the clip whatever the codecs, and the output open as
        `tmp` -> (ctx, fetch, store).  What the tool runs inside the block happens before the rename to `final`, what it runs after
        it after the rename; an exception from inside leaves no tmp file and goes on propagating."""
        import torch
        self.on_device(torch.device("cuda", torch.cuda.current_device()), *self.codecs, own_context=True)
        with torch.cuda.device(self.dev), ClipOutput(tmp, final, self.n, (self.H, self.W, 3), self.fps, self.codecs[1], self.ctx) as out:
            yield self.ctx, self.fetch, out.store


# ---- the list loop ------------------------------------------------------------------------------------------------------------------

def run_list(args, infer, check, load, run_clip, banner: str = "\n##### [{k}/{n}] Processing {path} #####"):
    """The body of every tool's run(args, infer): check(args) before any file is opened, the list is read, the generator is loaded
    once (load(), where infer is None), run_clip(args, path, infer) per clip in order -- a clip's exception ends the run -- with
    the banner for a list, even of one entry.  -> the written paths."""
    check(args)
    clips = clips_from_argument(args.color_video)
    if infer is None:
        infer = load()
    written = []
    for k, path in enumerate(clips, start=1):
        if is_txt(args.color_video):
            print(banner.format(k=k, n=len(clips), path=path))
        written.append(run_clip(args, path, infer))
    return written


# ---- the device wrappers' arguments -------------------------------------------------------------------------------------------------

def size_arg(size, what: str):
    """(width, height) as two ints, both at least 1."""
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise ValueError(f"{what} must be (width, height) with both at least 1, got {size!r}")
    return w, h


def non_empty(name: str, t, noun: str, dims=None):
    """The dims of a checked tensor (default: its first three) as a tuple, all at least 1: else `<name> holds no <noun>`."""
    dims = tuple(t.shape[:3] if dims is None else dims)
    if min(dims) < 1:
        raise ValueError(f"{name} holds no {noun}: shape {tuple(t.shape)}")
    return dims


def stream_or_current(dev, stream):
    import torch
    return torch.cuda.current_stream(dev) if stream is None else stream
