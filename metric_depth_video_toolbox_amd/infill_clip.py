"""What the four infill scripts (basic_nomal_infill, stereo_crafter_infill, m2svid_infill, stereo_dissoclusion_net_infill) share
one level above clip_io's frame I/O: the list-file arguments, the opening of a side-by-side clip with its checks and output names,
the black-padded mask fetch, the batch loop and the chunk loop, the chunk's per-eye skeleton and the command line's common flags
and tail.  A script configures these with what is its own: a prepare call, a generator contract and a finish call.

THE CHUNK SCHEDULE of the engines whose model sees a stretch of video (stereo_crafter_infill, m2svid_infill) is the reference's
(scr:218-266, m2s:398-453): 25 frames per chunk; after a chunk the buffer keeps six frames -- three pasted frames with their masks,
then three untouched ones; a chunk writes from its index 3 unless it is the first and stops 3 short unless it is the last; the last
call runs on whatever is buffered.  One difference, on purpose: the reference pairs the masks of the frames T-6 .. T-4 with the
pasted frames T-9 .. T-7 (its list of written frames is three short, so its [-6] is frame T-9: scr:148, 251-253, m2s:437-440); here
the pasted frames T-6 .. T-4 go with their own masks and their own further inputs.  Those three frames are context for the generator
only and are never written again.
"""
from __future__ import annotations

import importlib
import os
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from .clip_io import VIDEO_DECODERS, VIDEO_ENCODERS, ClipOutput, check_video_decoder, check_video_encoder, video_parts

FRAMES_CHUNK, OVERLAP = 25, 6             # scr:222, 250-257


# ---- list-file arguments ------------------------------------------------------------------------------------------------------------

def is_txt(path) -> bool:
    return isinstance(path, str) and path.lower().endswith(".txt")                      # bni:29-30


def read_list_file(path: str):
    """Stripped lines of a list file, blank lines and lines starting with '#' ignored (bni:32-43)."""
    with open(path, "r", encoding="utf-8") as f:
        return [ln.strip() for ln in f if ln.strip() and not ln.strip().startswith("#")]


def tuples_from_arguments(named):
    """bni:246-260, scr:343, m2s:494-507, sdn:238-250.  named: the (flag name, value) pairs of a script's clip arguments, the leading
    one first.  One tuple of the values, or -- if the leading value is a .txt list -- the tuples of as many lists of equal length.
    The lists are read and compared before any clip is opened."""
    values = [v for _, v in named]
    if not is_txt(values[0]):
        return [tuple(values)]
    if not all(is_txt(v) for v in values[1:]):
        rest = " and ".join(f"--{name}" for name, _ in named[1:])
        raise ValueError(f"If --{named[0][0]} is a .txt file, then {rest} must also be {'a .txt file' if len(named) == 2 else '.txt files'}.")
    lists = [read_list_file(v) for v in values]
    if any(len(entries) != len(lists[0]) for entries in lists):
        raise ValueError("List length mismatch: " + ", ".join(f"{v} has {len(entries)} entries" for v, entries in zip(values, lists)) + ".")
    return list(zip(*lists))


# ---- opening a side-by-side clip ----------------------------------------------------------------------------------------------------

class Clip(NamedTuple):
    """An opened side-by-side clip: what open_clip found out, and what the two loops need to write its output."""
    frames: tuple                 # the opened (colour, mask, *further inputs)
    n: int                        # frames to process
    video: bool                   # .mkv files (else .npy frame dumps)
    fps: Optional[float]          # the colour video's frame rate (bni:134); None for frame dumps
    tmp: str                      # `<sbs_color>_tmp_infilled.<ext>`: written, then renamed to
    final: str                    # `<sbs_color>_infilled.<ext>`
    encoder: str


def open_clip(inp, color_path: str, mask_path: str, extras, max_frames: int, video_decoder: str, video_encoder: str, device=None, *,
              zero_frames: str = "max_frames = 0: ask for -1 (all) or a positive count", allow_empty: bool = False) -> Clip:
    """The head of every process_pair (bni:124-145, scr:192-214, m2s:367-394, sdn:125-152), inside the block of the ClipInputs `inp`.
    extras: the further inputs as (argument name, path, run_output, what it means when it has fewer than n frames).  Colour, mask and
    every run_output input are outputs of clip.run (they may exist as per-rank segments + index: run_output reads either form) and
    must have the colour clip's frame size; any other input is some uint8 [N, H, W, 3] clip.  zero_frames / allow_empty:
    basic_nomal_infill words the first refusal differently and does not refuse a clip without frames."""
    import torch
    named = [("sbs_color_video", color_path, True, None), ("sbs_mask_video", mask_path, True, None)] + list(extras)
    frames = tuple(inp.open(path, name, Exception(f"input {name} does not exist: {path}"), run_output) for name, path, run_output, _ in named)
    color = frames[0]
    video = bool(video_parts(color))
    check_video_decoder(video_decoder, video)
    check_video_encoder(video_encoder, video)
    assert color.ndim == 4 and color.shape[-1] == 3 and color.dtype == np.uint8, "uint8 [N, H, 2W, 3] expected"
    for (name, _, run_output, _), f in zip(named[1:], frames[1:]):
        if run_output:
            assert color.shape[1:] == f.shape[1:], "mask and color video not same resolution"      # scr:210, m2s:390, sdn:147
        else:
            assert f.ndim == 4 and f.shape[-1] == 3 and f.dtype == np.uint8, f"uint8 [N, H, W, 3] expected for {name}"
    if color.shape[2] % 2:
        raise ValueError(f"side-by-side frames need an even width, got {color.shape[2]}")     # (the reference gives the right eye the odd column: bni:180-181)
    if max_frames == 0:
        raise ValueError(zero_frames)
    n = color.shape[0] if max_frames == -1 else min(color.shape[0], max_frames)
    if n < 1 and not allow_empty:
        raise ValueError(f"{color_path} has no frames")
    for (_, path, _, short), f in zip(named[2:], frames[2:]):
        if f.shape[0] < n:
            raise ValueError(f"{short}: {path} has {f.shape[0]} frames, {n} are needed")
    ext = ".mkv" if video else ".npy"
    fps = (video_parts(color)[0][0].fps or 30.0) if video else None
    inp.on_device(torch.device("cuda", torch.cuda.current_device() if device is None else device), video_decoder, video_encoder)
    # bni:140-141, scr:213-214, m2s:393-394, sdn:151-152: the names hang on the colour video's full name
    return Clip(frames, n, video, fps, color_path + "_tmp_infilled" + ext, color_path + "_infilled" + ext, video_encoder)


# ---- the mask, black where its clip has ended ---------------------------------------------------------------------------------------

def mask_split(a: int, b: int, mask_len: int):
    """Of the clip's frames [a, b): (how many the mask clip has, how many it has not: black masks, bni:165-167, scr:234-237,
    m2s:415-417, sdn:176-178)."""
    have = max(0, min(b, mask_len) - a)
    return have, b - a - have


def fetch_mask(inp, mask, a: int, b: int, out=None):
    """Frames [a, b) of the mask, black where the mask clip has ended: a fresh tensor, or written into `out` (b - a frames of a buffer)."""
    import torch
    have, blank = mask_split(a, b, mask.shape[0])
    if out is None:
        if not blank:
            return inp.fetch(mask, a, b)
        out = torch.zeros((b - a,) + tuple(mask.shape[1:]), dtype=torch.uint8, device=inp.dev)
    else:
        out[have:] = 0
    if have:
        out[:have] = inp.fetch(mask, a, a + have)
    return out


# ---- the two loops ------------------------------------------------------------------------------------------------------------------

def run_batches(inp, clip: Clip, batch: int, per_batch):
    """The frame-by-frame engines' loop: per batch of the clip, per_batch(colour, mask, *further inputs) -> the frames to store."""
    import torch
    color, mask, *extras = clip.frames
    batch = max(1, int(batch))
    with ClipOutput(clip.tmp, clip.final, clip.n, color.shape[1:], clip.fps, clip.encoder, inp.ctx) as out, torch.cuda.device(inp.dev):
        for a in range(0, clip.n, batch):
            b = min(a + batch, clip.n)
            d_color, d_extras = inp.fetch(color, a, b), [inp.fetch(x, a, b) for x in extras]
            out.store(per_batch(d_color, fetch_mask(inp, mask, a, b), *d_extras), a)


def chunk_schedule(n_frames: int, chunk: int = FRAMES_CHUNK):
    """The calls of the chunk schedule (above) for a clip of n_frames: [(first, last, frame of the buffer's index 0, buffered frames,
    (a, b))], where [a, b) are the clip's frames the call writes.  chunk: the frames per chunk (inspatio_world_infill: 225)."""
    if n_frames < 1:
        raise ValueError("a clip needs at least one frame")
    if chunk <= OVERLAP:
        raise ValueError(f"a chunk must be longer than the {OVERLAP} frames kept between chunks")
    calls, first, base, held = [], True, 0, 0
    for t in range(n_frames):
        held += 1
        if held >= chunk:
            start = 0 if first else 3
            calls.append((first, False, base, held, (base + start, base + held - 3)))
            first, base, held = False, base + held - OVERLAP, OVERLAP
    start = 0 if first else 3
    calls.append((first, True, base, held, (base + start, base + held)))
    return calls


def run_chunks(inp, clip: Clip, batch: int, per_chunk, store_blended: bool = True, chunk: int = FRAMES_CHUNK):
    """The chunk schedule (above) over the clip, read `batch` frames at a time: per call,
    per_chunk(first, last, fps, colour, mask, *further inputs) -> (start, pasted, blended) as infill_chunk returns them.  The file
    gets the blended frames or the pasted ones; the pasted ones feed the overlap either way (m2s:308, 332).  The generator is told
    30 frames per second for frame dumps.  chunk: the frames per chunk."""
    import torch
    color, mask, *extras = clip.frames
    batch = max(1, int(batch))
    fps = clip.fps if clip.video else 30.0
    with ClipOutput(clip.tmp, clip.final, clip.n, color.shape[1:], clip.fps, clip.encoder, inp.ctx) as out, torch.cuda.device(inp.dev):
        buf_c = torch.empty((chunk,) + tuple(int(v) for v in color.shape[1:]), dtype=torch.uint8, device=inp.dev)
        buf_m = torch.zeros_like(buf_c)
        buf_x = [torch.empty((chunk,) + tuple(int(v) for v in x.shape[1:]), dtype=torch.uint8, device=inp.dev) for x in extras]
        read = 0
        for first, last, base, held, (wa, wb) in chunk_schedule(clip.n, chunk):
            have = read - base                                     # the overlap is in the buffer already
            while have < held:
                k = min(batch, held - have)
                buf_c[have:have + k] = inp.fetch(color, read, read + k)
                for buf, x in zip(buf_x, extras):
                    buf[have:have + k] = inp.fetch(x, read, read + k)
                fetch_mask(inp, mask, read, read + k, out=buf_m[have:have + k])
                have += k
                read += k
            start, pasted, blended = per_chunk(first, last, fps, buf_c[:held], buf_m[:held], *(buf[:held] for buf in buf_x))
            assert base + start == wa and len(blended) == wb - wa
            if wb > wa:
                out.store(blended if store_blended else pasted, wa)      # m2s:310-329
            if not last:                                           # scr:250-257, m2s:437-444
                keep_c = torch.cat([pasted[held - OVERLAP - start:held - 3 - start], buf_c[held - 3:held]])
                keep = [buf[held - OVERLAP:held].clone() for buf in (buf_m, *buf_x)]
                buf_c[:OVERLAP] = keep_c
                for buf, kept in zip((buf_m, *buf_x), keep):
                    buf[:OVERLAP] = kept


# ---- one chunk: the device wrappers and the skeleton the chunked engines share ------------------------------------------------------

def frames4(t, channels=3, name="frames", shape=None, device=None, output=False, disjoint=True):
    """_lib.check_tensor for uint8 CUDA frames [N,H,W,3] (channels = 3) or planes [N,H,W] (channels = 1) with packed pixels, rows and
    frames padded at will but not overlapping (the adapter and engine entry points take no stride below a frame; disjoint=False: any
    stride); `shape` holds it to one size, `device` to a GPU (or a tensor's), `output` marks a tensor that is written."""
    import torch
    if shape is None:
        shape = (None, None, None, 3) if channels == 3 else (None, None, None)
    return _lib.check_tensor(name, t, torch.uint8, shape, device=device, packed=2 if channels == 3 else 1, output=output, disjoint=disjoint)


def composite_eye(model_frames, sbs_color, sbs_mask, eye: int, pasted, blended):
    """scr:151-188 (and, word for word, m2s:290-327) for one eye: the model's frames (uint8 CUDA [N,mh,mw,3]) resized back, pasted
    under the mask into that eye's half of `pasted` and blended along the holes' lower side into that eye's half of `blended` (both
    uint8 CUDA [N,H,2W,3]).  All on one GPU, pixels packed; rows and frames may be strided, those of pasted and blended without overlap."""
    frames4(sbs_color, name="sbs_color")
    N, H, W2 = (int(v) for v in sbs_color.shape[:3])
    if W2 % 2:
        raise ValueError(f"sbs_color must hold two eyes side by side, got a width of {W2}")
    frames4(model_frames, name="model_frames", shape=(N, None, None, 3), device=sbs_color)
    frames4(sbs_mask, name="sbs_mask", shape=tuple(sbs_color.shape), device=sbs_color)
    frames4(pasted, name="pasted", shape=tuple(sbs_color.shape), device=sbs_color, output=True)
    frames4(blended, name="blended", shape=tuple(sbs_color.shape), device=sbs_color, output=True)
    _lib.shared_context(sbs_color.device).call(
        "mdvt_adapter_composite_eye", W2 // 2, H, N, int(eye), model_frames.data_ptr(), int(model_frames.shape[2]), int(model_frames.shape[1]),
        model_frames.stride(1), model_frames.stride(0), sbs_color.data_ptr(), sbs_color.stride(1), sbs_color.stride(0),
        sbs_mask.data_ptr(), sbs_mask.stride(1), sbs_mask.stride(0), pasted.data_ptr(), pasted.stride(1), pasted.stride(0),
        blended.data_ptr(), blended.stride(1), blended.stride(0), _lib.stream_arg(sbs_color.device))


def checked_model_frames(frames, like):
    """What a generator returned, contiguous -- or the TypeError of the generator contracts: a uint8 CUDA tensor of `like`'s shape."""
    import torch
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.shape == like.shape):
        raise TypeError(f"the generator must return a uint8 CUDA tensor of shape {tuple(like.shape)}")
    return frames.contiguous()


def infill_chunk(keep_first_three: bool, keep_last_three: bool, color, mask, prepare, generate, finish=None):
    """scr:91-190, m2s:211-332 on a chunk of uint8 CUDA [T,H,2W,3] colour and mask frames.  Per eye: prepare(eye) -> (image,
    *model inputs, hole counts); where there are holes, generate(image, *model inputs) -> the model's frames, then -- if given --
    finish(frames, image, *model inputs) -> frames; composite_eye.  Returns (first, pasted, blended): the chunk's index of the first
    frame it writes and the pasted and blended frames from there to the last one it writes (scr:147-148)."""
    import torch
    T = int(color.shape[0])
    start = 0 if keep_first_three else 3
    end = T if keep_last_three else T - 3
    n = max(end - start, 0)
    pasted = torch.empty((n,) + tuple(color.shape[1:]), dtype=torch.uint8, device=color.device)
    blended = torch.empty_like(pasted)
    for eye in (0, 1):                                             # scr:133-145, m2s:270-284: the left eye first
        image, *model_inputs, counts = prepare(eye)
        if int(counts.sum().item()) == 0:                          # scr:134, 141, m2s:271, 280: no holes, no model
            frames = image
        else:
            frames = checked_model_frames(generate(image, *model_inputs), image)
            if finish is not None:
                frames = finish(frames, image, *model_inputs)
        if n:
            composite_eye(frames[start:end], color[start:end], mask[start:end], eye, pasted, blended)
    return start, pasted, blended


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def callable_from_spec(spec: str, default_name: str):
    """The callable a `--generator pkg.module:callable` names (default_name: the engine's own model, for the message)."""
    mod, sep, name = spec.partition(":")
    if not sep or not mod or not name:
        raise ValueError(f"--generator must be '{default_name}' or 'pkg.module:callable', got {spec!r}")
    fn = getattr(importlib.import_module(mod), name, None)
    if not callable(fn):
        raise ValueError(f"{spec}: {mod} has no callable {name!r}")
    return fn


def add_common_flags(p):
    """--max_frames (the reference's) and the three flags that are not: --batch, --video_decoder, --video_encoder."""
    p.add_argument("--max_frames", default=-1, type=int, help="quit after max_frames nr of frames", required=False)
    p.add_argument("--batch", default=8, type=int, help="not a reference flag: frames per read from the inputs (and per device batch, where the engine works frame by frame)")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="not a reference flag: where the .mkv inputs are FFV1-decoded -- 'host' (default) or 'device' (on the GPU, the "
                        "same bytes; only the compressed packets are copied to the device; a stream the device does not decode is "
                        "read on the host) or 'device_all' (as 'device', and Golomb-Rice or inter-coded FFV1, FFmpeg's default, is "
                        "decoded on the GPU as well). Not with .npy inputs")
    p.add_argument("--video_encoder", choices=VIDEO_ENCODERS, default="host",
                   help="not a reference flag: where the .mkv output is FFV1-encoded -- 'host' (default) or 'device' (on the GPU, the "
                        "same bytes). Not with .npy inputs")
    return p


def run_clips(named, max_frames: int, process, precheck=None, load=None) -> int:
    """The tail of every main (bni:246-274, scr:343-354, m2s:494-520, sdn:238-263).  named: as for tuples_from_arguments;
    process(paths, generate) -> the output path of one clip.  precheck: per argument, whether it may also exist as `<path>.index.json`
    (clip_io.open_frames' run_output) -- given, --max_frames 0 and a single clip's missing file end the run before the model is
    loaded; basic_nomal_infill gives none.  load: makes the generator, once; its RuntimeError, ValueError or ImportError ends the run."""
    if precheck is not None and max_frames == 0:
        raise SystemExit("--max_frames 0: ask for -1 (all) or a positive count")
    clips = tuples_from_arguments(named)
    listed = is_txt(named[0][1])
    if precheck is not None and not listed:
        for (name, path), run_output in zip(named, precheck):
            if not (os.path.isfile(path) or (run_output and os.path.isfile(path + ".index.json"))):
                raise SystemExit(f"input {name} does not exist: {path}")
    generate = None
    if load is not None:
        try:
            generate = load()
        except (RuntimeError, ValueError, ImportError) as e:
            raise SystemExit(str(e))
    if not listed:
        print("Done. Wrote:", process(clips[0], generate))
        return 0
    # (the reference runs two clips at a time with the GPU sections or the model serialised, bni:262-274, scr:343-354, m2s:509-520,
    #  sdn:252-263; here a clip is I/O and one launch set per batch or chunk, so the clips simply follow each other)
    print(f"Batch mode: {len(clips)} pairs")
    for paths in clips:
        try:
            print("Done. Wrote:", process(paths, generate))
        except Exception as e:                                     # bni:270-274, scr:352-354, m2s:518-520, sdn:261-263: surface the error, keep the other clips going
            print(f"[ERROR] A clip failed: {e}")
    return 0
