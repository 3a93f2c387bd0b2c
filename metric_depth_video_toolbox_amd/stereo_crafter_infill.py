"""Device-side mirror of the reference's stereo_crafter_infill.py ("scr"; movie_2_3D.py's default --infill_engine): the same
names and argument meaning, on PyTorch-ROCm tensors through libmdvt_hip.so (include/mdvt_infill_adapter.h).  No CPU fallback.

    transfer_lhm_video_refmask(video, reference, reference_mask)     infill_common.py:52-130, on device tensors
    deal_with_frame_chunk(...)                                       scr:91-190, one chunk of side-by-side frames
    process_pair(sbs_color, sbs_mask, generate)                      scr:192-274, on the clip driver's outputs
    python -m metric_depth_video_toolbox_amd.stereo_crafter_infill --sbs_color_video X.mkv --sbs_mask_video Y.mkv

The in-painting model is a callable, THE GENERATOR CONTRACT:

    generate(frames, masks, fps) -> frames

frames: uint8 CUDA tensor [T, 768, 1024, 3] (RGB; the left eye mirrored), masks: uint8 CUDA tensor [T, 768, 1024] (255 = fill here),
fps: the clip's frame rate.  Returns a uint8 CUDA tensor of the shape of `frames`, produced on the current stream.  `--generator
pkg.module:callable` names one; the default, `stereocrafter`, wraps StereoCrafter's pipeline with the reference's arguments
(scr:57-82) and needs StereoCrafter, diffusers and transformers, none of which this project ships or tests against.

Everything around the model runs on the device: the eyes are split, mirrored and resized (mdvt_adapter_prepare_eye), the model's
colours matched to its input (mdvt_lhm_moments -> the float64 host algebra of lhm_params on 30 integers per frame -> mdvt_lhm_apply),
the frames resized back, pasted under the mask and blended along the holes' lower side (mdvt_adapter_composite_eye).  The colour
match follows the reference's single_precision=False; its default float32 path differs from that in a few per cent of the values by
1 (include/mdvt_infill_adapter.h).

The chunk schedule is the reference's (scr:218-266), with its one difference on purpose; infill_clip describes it and runs it
(chunk_schedule, run_chunks), and owns composite_eye, which m2svid_infill uses too: both are re-exported here.
"""
from __future__ import annotations

import argparse

import numpy as np

from . import _lib
from .clip_io import ClipInputs
from .infill_clip import (FRAMES_CHUNK, OVERLAP, add_common_flags, callable_from_spec, chunk_schedule, composite_eye, frames4,      # noqa: F401
                          infill_chunk, open_clip, run_chunks, run_clips)

MODEL_W, MODEL_H = 1024, 768              # scr:95-96
EPS = 1e-5                                # ic:57


def prepare_eye(sbs_color, sbs_mask, eye: int, model_size=(MODEL_W, MODEL_H)):
    """scr:101-126 for one eye (0 = left, read mirrored; 1 = right) of uint8 CUDA [N,H,2W,3] colour and infill-mask frames ->
    (image [N,mh,mw,3], mask [N,mh,mw], hole counts int32 [N]), all on the device."""
    import torch
    frames4(sbs_color, name="sbs_color"), frames4(sbs_mask, name="sbs_mask", shape=tuple(sbs_color.shape), device=sbs_color)
    if sbs_color.shape[2] % 2:
        raise ValueError(f"sbs_color must hold two eyes side by side, got a width of {int(sbs_color.shape[2])}")
    N, H, W2 = (int(v) for v in sbs_color.shape[:3])
    mw, mh = model_size
    image = torch.empty((N, mh, mw, 3), dtype=torch.uint8, device=sbs_color.device)
    mask = torch.empty((N, mh, mw), dtype=torch.uint8, device=sbs_color.device)
    counts = torch.empty((N,), dtype=torch.int32, device=sbs_color.device)
    _lib.shared_context(sbs_color.device).call(
        "mdvt_adapter_prepare_eye", W2 // 2, H, N, int(eye), sbs_color.data_ptr(), sbs_color.stride(1), sbs_color.stride(0),
        sbs_mask.data_ptr(), sbs_mask.stride(1), sbs_mask.stride(0), mw, mh, image.data_ptr(), image.stride(1), image.stride(0),
        mask.data_ptr(), mask.stride(1), mask.stride(0), counts.data_ptr(), _lib.stream_arg(sbs_color.device))
    return image, mask, counts


def lhm_moments(frames, mask=None, out=None):
    """mdvt_lhm_moments: per frame of uint8 CUDA [N,H,W,3] the ten exact integer moments (count, sums, second moments) over the
    pixels whose mask byte is 0 (all without a mask) -> int64 CUDA [N,10]."""
    import torch
    frames4(frames)
    N, H, W = (int(v) for v in frames.shape[:3])
    if mask is not None:
        frames4(mask, 1, name="mask", shape=(N, H, W), device=frames)
    if out is None:
        out = torch.empty((N, 10), dtype=torch.int64, device=frames.device)
    _lib.check_tensor("out", out, torch.int64, (N, 10), device=frames, contiguous=True)
    _lib.shared_context(frames.device).call(
        "mdvt_lhm_moments", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0),
        mask.data_ptr() if mask is not None else None, mask.stride(1) if mask is not None else 0, mask.stride(0) if mask is not None else 0,
        out.data_ptr(), _lib.stream_arg(frames.device))
    return out


def _mean_cov(m):
    """Ten integer moments -> (mu, cov + eps on the diagonal) in float64; the covariance's numerator is formed exactly in integers."""
    n, s1 = int(m[0]), [int(v) for v in m[1:4]]
    q = [int(v) for v in m[4:10]]
    s2 = [[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]]
    mu = np.array(s1, dtype=np.float64) / n
    den = float(n) * max(n - 1, 1)
    cov = np.array([[float(n * s2[i][j] - s1[i] * s1[j]) / den for j in range(3)] for i in range(3)], dtype=np.float64)
    cov = 0.5 * (cov + cov.T)
    cov[np.arange(3), np.arange(3)] += EPS
    return mu, cov


def lhm_params(mom_x, mom_r, mom_r_all):
    """The host algebra of the colour match (ic:100-125), float64, per frame: the moments of the video frame, of the reference's
    kept pixels and of all the reference's pixels (used where fewer than 3 are kept, ic:113-114) -> [N,15] float64: A row-major,
    mu_x, mu_r."""
    out = np.empty((len(mom_x), 15), dtype=np.float64)
    for k in range(len(mom_x)):
        mu_x, cov_x = _mean_cov(mom_x[k])
        eval_x, evec_x = np.linalg.eigh(cov_x)
        invsqrt_x = (evec_x * (1.0 / np.sqrt(np.clip(eval_x, EPS, None)))) @ evec_x.T
        mu_r, cov_r = _mean_cov(mom_r[k] if int(mom_r[k][0]) >= 3 else mom_r_all[k])
        eval_r, evec_r = np.linalg.eigh(cov_r)
        sqrt_r = (evec_r * np.sqrt(np.clip(eval_r, 0, None))) @ evec_r.T
        out[k, :9] = (sqrt_r @ invsqrt_x).reshape(9)
        out[k, 9:12] = mu_x
        out[k, 12:] = mu_r
    return out


def lhm_apply(frames, params, out=None):
    """mdvt_lhm_apply: uint8 CUDA [N,H,W,3] (rows and frames may be strided) and contiguous float64 CUDA [N,15] -> the matched
    frames; out, where given: uint8 [N,H,W,3] on the same GPU, pixels packed, rows and frames strided without overlap."""
    import torch
    frames4(frames)
    N, H, W = (int(v) for v in frames.shape[:3])
    _lib.check_tensor("params", params, torch.float64, (N, 15), device=frames, contiguous=True)
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=frames.device)
    frames4(out, name="out", shape=(N, H, W, 3), device=frames, output=True)
    _lib.shared_context(frames.device).call("mdvt_lhm_apply", W, H, N, frames.data_ptr(), frames.stride(1), frames.stride(0), params.data_ptr(),
                                            out.data_ptr(), out.stride(1), out.stride(0), _lib.stream_arg(frames.device))
    return out


def transfer_lhm_video_refmask(video, reference, reference_mask=None):
    """infill_common.transfer_lhm_video_refmask (ic:52-130) with single_precision=False, on uint8 CUDA tensors: video [T,H,W,3],
    reference [H,W,3] or [T,H,W,3], reference_mask None, [H,W] or [T,H,W] (0 = the pixel counts).  One small read-back (the
    3 x T x 10 moments) per call."""
    import torch
    assert video.dim() == 4, "video must be (T,H,W,C)"
    T = int(video.shape[0])
    if reference.dim() == 3:
        reference = reference.unsqueeze(0).expand(T, -1, -1, -1).contiguous()
    assert reference.shape == video.shape, "reference must be (H,W,C) or (T,H,W,C) of the video's size"
    mom = torch.empty((3, T, 10), dtype=torch.int64, device=video.device)
    lhm_moments(video, None, out=mom[0])
    lhm_moments(reference, None, out=mom[2])
    if reference_mask is None:
        mom[1].copy_(mom[2])
    else:
        if reference_mask.dim() == 2:
            reference_mask = reference_mask.unsqueeze(0).expand(T, -1, -1).contiguous()
        lhm_moments(reference, reference_mask, out=mom[1])
    m = mom.cpu().numpy()
    params = torch.from_numpy(lhm_params(m[0], m[1], m[2])).to(video.device)
    return lhm_apply(video, params)


def deal_with_frame_chunk(keep_first_three: bool, color, mask, keep_last_three: bool, fps: float, generate, model_size=(MODEL_W, MODEL_H)):
    """scr:91-190 on a chunk of uint8 CUDA [T,H,2W,3] colour and mask frames.  Returns (first, pasted, blended): the chunk's index of
    the first frame it writes and the pasted and blended frames from there to the last one it writes (scr:147-148)."""
    return infill_chunk(keep_first_three, keep_last_three, color, mask, lambda eye: prepare_eye(color, mask, eye, model_size),
                        lambda image, mmask: generate(image, mmask, fps), transfer_lhm_video_refmask)


def process_pair(sbs_color_video_path: str, sbs_mask_video_path: str, generate, max_frames: int = -1, batch: int = 8, device=None, *,
                 video_decoder: str = "host", video_encoder: str = "host", model_size=(MODEL_W, MODEL_H)):
    """scr:192-274.  `.mkv` inputs give `<sbs_color>_infilled.mkv` at the colour video's frame rate, frame dumps (`.npy`, uint8
    [N,H,2W,3]) give `<sbs_color>_infilled.npy`; either is written under its `_tmp_infilled` name and renamed once every frame is in.
    A mask clip shorter than the colour clip means black masks for the rest (scr:234-237).  Returns the output path."""
    with ClipInputs() as inp:
        clip = open_clip(inp, sbs_color_video_path, sbs_mask_video_path, [], max_frames, video_decoder, video_encoder, device)
        run_chunks(inp, clip, batch, lambda first, last, fps, color, mask: deal_with_frame_chunk(first, color, mask, last, fps, generate, model_size))
    return clip.final


class StereoCrafterGenerator:
    """The default generator: StereoCrafter's in-painting pipeline with the reference's arguments (scr:57-82, 291-325).  Needs the
    StereoCrafter checkout, diffusers and transformers and their weights; UNTESTED here (none of them is available to this project)."""

    def __init__(self, num_inference_steps: int = 5, img2vid_path: str = "weights/stable-video-diffusion-img2vid-xt-1-1",
                 unet_path: str = "StereoCrafter/weights/StereoCrafter"):
        try:
            import torch
            from diffusers import AutoencoderKLTemporalDecoder, UNetSpatioTemporalConditionModel
            from transformers import CLIPVisionModelWithProjection
            from StereoCrafter.pipelines.stereo_video_inpainting import StableVideoDiffusionInpaintingPipeline, tensor2vid
        except ImportError as e:
            raise RuntimeError(f"the stereocrafter generator needs StereoCrafter, diffusers and transformers ({e}); "
                               "install them or name another model with --generator pkg.module:callable") from None
        half = dict(torch_dtype=torch.float16)
        encoder = CLIPVisionModelWithProjection.from_pretrained(img2vid_path, subfolder="image_encoder", variant="fp16", **half)
        vae = AutoencoderKLTemporalDecoder.from_pretrained(img2vid_path, subfolder="vae", variant="fp16", **half)
        unet = UNetSpatioTemporalConditionModel.from_pretrained(unet_path, subfolder="unet_diffusers", low_cpu_mem_usage=True, **half)
        for m in (encoder, vae, unet):
            m.requires_grad_(False)
        self.pipeline = StableVideoDiffusionInpaintingPipeline.from_pretrained(img2vid_path, image_encoder=encoder, vae=vae, unet=unet,
                                                                              **half).to("cuda")
        self.tensor2vid, self.steps = tensor2vid, int(num_inference_steps)

    def __call__(self, frames, masks, fps):
        import torch
        x = frames.permute(0, 3, 1, 2).float() / 255.0
        m = masks.float() / 255.0
        latents = self.pipeline(frames=x, frames_mask=m, height=x.shape[2], width=x.shape[3], num_frames=len(x), output_type="latent",
                                min_guidance_scale=1.01, max_guidance_scale=1.01, decode_chunk_size=8, fps=fps, motion_bucket_id=127,
                                noise_aug_strength=0.0, num_inference_steps=self.steps).frames[0].unsqueeze(0)
        decoded = self.pipeline.decode_latents(latents, num_frames=latents.shape[1], decode_chunk_size=2)
        video = self.tensor2vid(decoded, self.pipeline.image_processor, output_type="np")[0]
        return torch.from_numpy((video * 255).astype(np.uint8)).to(frames.device)


def load_generator(spec: str, num_inference_steps: int = 5):
    """`stereocrafter` (the default model) or `pkg.module:callable`."""
    return StereoCrafterGenerator(num_inference_steps) if spec == "stereocrafter" else callable_from_spec(spec, "stereocrafter")


def build_parser():
    p = argparse.ArgumentParser(description="StereoCrafter infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--sbs_color_video", type=str, required=True, help="side by side stereo video rendered with point clouds in the masked area (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="side by side stereo video mask, or the matching .txt list")
    p.add_argument("--num_inference_steps", default=5, type=int, help="number of diffusion steps of the stereocrafter generator. More look better but is slower", required=False)
    p.add_argument("--generator", default="stereocrafter", type=str,
                   help="not a reference flag: the in-painting model, 'stereocrafter' (default) or pkg.module:callable with "
                        "generate(frames, masks, fps) -> frames on uint8 CUDA tensors [T,768,1024,3] and [T,768,1024]")
    return add_common_flags(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = dict(batch=args.batch, video_decoder=args.video_decoder, video_encoder=args.video_encoder)
    return run_clips([("sbs_color_video", args.sbs_color_video), ("sbs_mask_video", args.sbs_mask_video)], args.max_frames,
                     lambda paths, generate: process_pair(*paths, generate, args.max_frames, **kw), precheck=(True, True),
                     load=lambda: load_generator(args.generator, args.num_inference_steps))


if __name__ == "__main__":
    import sys
    sys.exit(main())
