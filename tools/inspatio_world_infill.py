#!/usr/bin/env python3
"""The reference's inspatio_world_infill.py ("iwi"; movie_2_3D.py's --infill_engine inspatio_world) around its video model, on the GPU:

    python tools/inspatio_world_infill.py --color_video x.mkv|list.txt --sbs_color_video x.mkv_stereo.mkv --sbs_mask_video
        x.mkv_stereo.mkv_infillmask.mkv [--max_frames N --apply_edge_blending --text_prompt T --batch 8
        --video_decoder host|device|device_all --video_encoder host|device] --generator pkg.module:callable

writes `<sbs_color>_infilled.mkv` (under its `_tmp_infilled` name first, renamed once every frame is in and the count is verified;
`.npy` frame dumps give `.npy`).  With `.txt` lists, all three arguments must be lists of equal length.

THE GENERATOR CONTRACT:

    generate(source, render, mask, fps, text_prompt) -> frames

source: uint8 CUDA [T, 480, 832, 3], the original frames at the model's size (shared by both eyes); render: uint8 CUDA [T, 480, 832, 3],
the eye's render with its holes black; mask: uint8 CUDA [T, 480, 832], the eye's validity plane resized (255 = keep, 0 = hole, values
between at the holes' rims: it is not thresholded); fps: the clip's frame rate; text_prompt: the scene's description.  T is already
padded to a count the model takes (inspatio_world.pad_to_valid_T) by repeating the last frame; the step trims the result.  Returns a
uint8 CUDA tensor [T, 480, 832, 3].  The float conversion, the latents and the shared source latent are the wrapper's business.  The
default, `inspatio_world`, wraps the InSpatio-World pipeline as the reference does (iwi:258-361, 659-723); it imports the model
lazily, fails with one line without it, and is UNTESTED (neither the checkout nor its weights are available to this project).

Per chunk (225 frames, 6 kept: infill_clip's schedule, the pasted frames with their own masks) and eye, everything but the model on
the device (include/mdvt_inspatio.h; wrappers: metric_depth_video_toolbox_amd/inspatio_device.py): mdvt_inspatio_prepare_eye, the model skipped where the
chunk's eye has no hole (iwi:446, 452), its frames resized back (mdvt_inspatio_model_frames), mdvt_masked_shift_grid, the grid
clean-up on the host (inspatio_world.flow_grids), mdvt_flow_warp, mdvt_inspatio_composite_eye.  Read-backs: the hole counts of both
eyes once per chunk, then per eye with holes the shifts and status bytes; one upload per such eye: the float32 grids.

NOT WIRED INTO THE DRIVER: movie_2_3D keeps refusing --infill_engine inspatio_world (that refusal and its text are held by existing
tests); wiring the engine in is a follow-up.  Refused: --lower_mask_dilation other than 0 (NotImplementedError: it repaints the render
and changes the masks before the model, iwi:392-397, and the driver never passes it); a colour video shorter than the side-by-side
video (ValueError before an output is opened, iwi:583-585)."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from metric_depth_video_toolbox_amd import _lib, inspatio_world as iw                                  # noqa: E402
from metric_depth_video_toolbox_amd.clip_io import ClipInputs                                          # noqa: E402
from metric_depth_video_toolbox_amd.infill_clip import add_common_flags, callable_from_spec, open_clip, run_chunks, run_clips      # noqa: E402

MODEL_W, MODEL_H = 832, 480               # iwi: TARGET_WIDTH, TARGET_HEIGHT
TEXT_PROMPT = "A realistic video of a scene"
DILATION_REASON = ("--lower_mask_dilation is left out: it repaints the render red and moves the holes' lower side before the model "
                   "(iwi:392-397), which none of the device calls of this step does; the driver never passes it")


def _padded(t, T):
    """t [n, ...] -> [T, ...] by repeating the last frame (iwi:298-301)."""
    import torch
    n = int(t.shape[0])
    return t if n == T else torch.cat([t, t[-1:].expand((T - n,) + tuple(t.shape[1:]))]).contiguous()


def deal_with_frame_chunk(keep_first_three, color, mask, org, keep_last_three, fps, generate, *, text_prompt=TEXT_PROMPT,
                          apply_edge_blending=False, model_size=(MODEL_W, MODEL_H)):
    """iwi:369-522 on a chunk of uint8 CUDA [T, H, 2W, 3] colour and mask frames and [T, oh, ow, 3] original frames.  Returns (first,
    pasted, blended): the chunk's index of the first frame it writes and the pasted and the blended frames (the pasted ones again
    without blending) from there to the last one it writes."""
    import numpy as np
    import torch
    from metric_depth_video_toolbox_amd import inspatio_device as idev
    dev = color.device
    ctx = _lib.shared_context(dev)
    T = int(color.shape[0])
    start, end = (0 if keep_first_three else 3), (T if keep_last_three else T - 3)
    n = max(end - start, 0)
    pasted = torch.empty((n,) + tuple(color.shape[1:]), dtype=torch.uint8, device=dev)
    blended = torch.empty_like(pasted) if apply_edge_blending else None
    eyes = [idev.prepare_eye(ctx, color, mask, eye, model_size) for eye in (0, 1)]
    holes = torch.stack([e[4] for e in eyes]).cpu().numpy()        # the chunk's first read-back: [2, T]
    Tp = iw.pad_to_valid_T(T)
    source = _padded(idev.model_frames(ctx, org, model_size), Tp) if holes.any() else None      # iwi:428-443: shared by both eyes
    for eye in (0, 1):                                             # iwi:445-455: the left eye first
        valid, render, m_valid, m_render, _ = eyes[eye]
        if not holes[eye].any():                                   # iwi:446, 452: no hole in the chunk's eye, no model, nothing to align
            aligned = render
        else:
            want = (Tp, model_size[1], model_size[0], 3)
            frames = generate(source, _padded(m_render, Tp), _padded(m_valid, Tp), fps, text_prompt)
            if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == want):
                raise TypeError(f"the generator must return a uint8 CUDA tensor of shape {want}")
            back = idev.model_frames(ctx, frames[:T].contiguous(), (int(valid.shape[2]), int(valid.shape[1])))      # iwi:347, 356-359
            shift, status, _ = idev.masked_shift_grid(ctx, render, back, valid)
            grids, has = iw.flow_grids(shift.cpu().numpy(), status.cpu().numpy(), holes[eye])                      # the eye's read-back
            aligned = idev.flow_warp(ctx, torch.from_numpy(np.ascontiguousarray(grids)).to(dev), torch.from_numpy(has).to(dev), back)
        if n:
            idev.composite_eye(ctx, aligned[start:end], color[start:end], mask[start:end], eye, pasted, blended)
    return start, pasted, (pasted if blended is None else blended)


def process_pair(sbs_color_video_path, sbs_mask_video_path, color_video_path, generate, max_frames=-1, batch=8, device=None, *,
                 apply_edge_blending=False, text_prompt=TEXT_PROMPT, video_decoder="host", video_encoder="host",
                 model_size=(MODEL_W, MODEL_H), chunk=iw.FRAMES_CHUNK):
    """iwi:528-627.  Returns the output path.  chunk: the frames per chunk (225; tests take less)."""
    with ClipInputs() as inp:
        clip = open_clip(inp, sbs_color_video_path, sbs_mask_video_path,
                         [("color_video", color_video_path, False, "Original color video ended before SBS video")], max_frames, video_decoder, video_encoder, device)
        run_chunks(inp, clip, batch, lambda first, last, fps, color, mask, org: deal_with_frame_chunk(
            first, color, mask, org, last, fps, generate, text_prompt=text_prompt, apply_edge_blending=apply_edge_blending, model_size=model_size),
            store_blended=True, chunk=chunk)
    return clip.final


class InspatioWorldGenerator:
    """The default generator: the InSpatio-World pipeline with the reference's conversions (iwi:242-252, 303-347) and set-up
    (iwi:659-723).  Needs the inspatio-world checkout, omegaconf, safetensors and the weights; UNTESTED here (none of them is
    available to this project).  The source latent is encoded once per distinct source tensor and kept for the other eye."""

    def __init__(self, root="inspatio-world"):
        try:
            if os.path.abspath(root) not in sys.path:
                sys.path.append(os.path.abspath(root))
            import torch
            import torch.distributed as dist
            from omegaconf import OmegaConf
            from safetensors.torch import load_file
            from pipeline import CausalInferencePipeline
            from utils.mask_utils import convert_mask_video
            from utils.memory import DynamicSwapInstaller
        except ImportError as e:
            raise RuntimeError(f"the inspatio_world generator needs the inspatio-world checkout, omegaconf and safetensors ({e}); "
                               "install them or name another model with --generator pkg.module:callable") from None
        dist.is_initialized, dist.get_rank = (lambda: True), (lambda *a, **k: 0)                # iwi:689-693: single process
        dist.get_world_size, dist.barrier = (lambda *a, **k: 1), (lambda *a, **k: None)
        config = OmegaConf.merge(OmegaConf.load(os.path.join(root, "configs", "default_config.yaml")), OmegaConf.load(os.path.join(root, "configs", "inference_1.3b.yaml")))
        config.wan_model_folder = os.path.join(root, "checkpoints", "Wan2.1-T2V-1.3B")
        for w in config.get("generator", {}).get("weight_list", []):
            if w.get("path", "").startswith("./"):
                w["path"] = os.path.join(root, w["path"][2:])
        dev = torch.device("cuda")
        pipe = CausalInferencePipeline(config, device=dev)
        pipe.generator.load_state_dict(load_file(os.path.join(root, "checkpoints", "InSpatio-World-1.3B", "InSpatio-World-1.3B.safetensors")), strict=False)
        pipe = pipe.to(dtype=torch.bfloat16)
        DynamicSwapInstaller.install_model(pipe.text_encoder, device=dev)
        pipe.vae.to(device=dev)
        pipe.generator.to(device=dev)
        torch.set_grad_enabled(False)
        pipe._initialize_kv_cache(batch_size=1, dtype=torch.bfloat16, device=dev)
        self.pipe, self.convert_mask, self.dev, self.ref = pipe, convert_mask_video, dev, (None, None)

    def __call__(self, source, render, mask, fps, text_prompt):
        import torch
        dt = torch.bfloat16

        def video(t):                                              # [T, H, W, 3] u8 -> [1, 3, T, H, W] in -1 .. 1 (iwi:242-245)
            return (t.float() / 127.5 - 1.0).permute(3, 0, 1, 2).unsqueeze(0).to(self.dev, dt)
        vae = self.pipe.vae
        render_latent = vae.encode_to_latent(video(render)).to(dt)
        vae.model.clear_cache()
        m = (mask.float() / 127.5 - 1.0)[None, None].expand(-1, 3, -1, -1, -1).to(self.dev, dt)      # iwi:248-252
        mask_latent = self.convert_mask(m).to(dt)
        if self.ref[0] is not source:                              # iwi:428-443: one source latent for both eyes
            self.ref = (source, vae.encode_to_latent(video(source)).to(dt))
            vae.model.clear_cache()
        ref = self.ref[1]
        noise = torch.randn([1, ref.shape[1], 16, ref.shape[3], ref.shape[4]], device=self.dev, dtype=dt)
        latents = self.pipe.inference(noise=noise, text_prompts=[text_prompt], ref_latent=ref, render_latent=render_latent, mask_latent=mask_latent, decode=False)
        out = (vae.decode_to_pixel(latents, use_cache=False) * 0.5 + 0.5).clamp(0, 1)
        vae.model.clear_cache()
        frames = (out[0].permute(0, 2, 3, 1).float() * 255).clamp(0, 255).to(torch.uint8)            # iwi:345-346: truncation
        T = int(render.shape[0])
        return (frames[:T] if frames.shape[0] >= T else _padded(frames, T)).contiguous()


def load_generator(spec):
    """`inspatio_world` (the default model) or `pkg.module:callable`."""
    return InspatioWorldGenerator() if spec == "inspatio_world" else callable_from_spec(spec, "inspatio_world")


def build_parser():
    p = argparse.ArgumentParser(description="InSpatio-World stereo infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--color_video", type=str, required=True, help="Original source video (single-eye width), or a .txt list of them")
    p.add_argument("--sbs_color_video", type=str, required=True, help="Side-by-side rendered video (left|right), or the matching .txt list")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="Side-by-side mask video (white = hole to fill), or the matching .txt list")
    p.add_argument("--apply_edge_blending", action="store_true", help="Blend edges to reduce halo artifacts")
    p.add_argument("--lower_mask_dilation", type=int, default=0, help="refused unless 0 (the reference's dilation of the holes' lower side before the model)")
    p.add_argument("--text_prompt", type=str, default=TEXT_PROMPT, help="Text description of the scene (generic prompt works fine)")
    p.add_argument("--generator", default="inspatio_world", type=str,
                   help="not a reference flag: the video model, 'inspatio_world' (default) or pkg.module:callable with "
                        "generate(source, render, mask, fps, text_prompt) -> frames on uint8 CUDA tensors [T,480,832,3], [T,480,832,3], [T,480,832]")
    p.add_argument("--chunk", type=int, default=iw.FRAMES_CHUNK, help="not a reference flag: frames per chunk (225, what the model was trained on)")
    return add_common_flags(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.lower_mask_dilation != 0:
        raise NotImplementedError(DILATION_REASON)
    if args.chunk <= iw.OVERLAP:
        raise ValueError(f"--chunk must be above the {iw.OVERLAP} frames kept between chunks, got {args.chunk}")
    kw = dict(batch=args.batch, apply_edge_blending=args.apply_edge_blending, text_prompt=args.text_prompt, video_decoder=args.video_decoder,
              video_encoder=args.video_encoder, chunk=args.chunk)
    return run_clips([("sbs_color_video", args.sbs_color_video), ("sbs_mask_video", args.sbs_mask_video), ("color_video", args.color_video)],
                     args.max_frames, lambda paths, generate: process_pair(*paths, generate, args.max_frames, **kw), precheck=(True, True, False),
                     load=lambda: load_generator(args.generator))


if __name__ == "__main__":
    sys.exit(main())
