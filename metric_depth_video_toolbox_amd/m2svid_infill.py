"""Device-side mirror of the reference's m2svid_infill.py ("m2s"; movie_2_3D.py's --infill_engine m2svid): the same names and
argument meaning, on PyTorch-ROCm tensors through libmdvt_hip.so (include/mdvt_infill_engines.h, include/mdvt_infill_adapter.h).
No CPU fallback.

    prepare_eye(sbs_color, sbs_mask, org, eye)                       m2s:224-261, the three model inputs of one eye
    deal_with_frame_chunk(...)                                       m2s:211-332, one chunk of side-by-side frames
    process_pair(sbs_color, sbs_mask, color, generate)               m2s:367-461, on the clip driver's outputs
    python -m metric_depth_video_toolbox_amd.m2svid_infill --color_video X.mkv --sbs_color_video Y.mkv --sbs_mask_video Z.mkv

The in-painting model is a callable, THE GENERATOR CONTRACT:

    generate(frames, masks, org_frames, fps) -> frames

frames: uint8 CUDA tensor [T, 512, 512, 3] (RGB; the rendered eye, the left eye mirrored), masks: uint8 CUDA tensor [T, 64, 64]
(255 = fill here), org_frames: uint8 CUDA tensor [T, 512, 512, 3] (the original frame, mirrored with the left eye), fps: the clip's
frame rate.  Returns a uint8 CUDA tensor of the shape of `frames`, produced on the current stream.  `--generator
pkg.module:callable` names one; the default, `m2svid`, wraps the m2svid model with the reference's float conversion and batch layout
(m2s:58-114) and needs the m2svid checkout, omegaconf and its weights, none of which this project ships or tests against.

Everything around the model runs on the device: the eyes are split, mirrored and resized together with the original frame and the
coarse mask (mdvt_m2svid_prepare_eye), the model's frames are resized back, pasted under the mask and blended along the holes' lower
side (mdvt_adapter_composite_eye: m2s:290-327 is, word for word, the arithmetic that call implements for the StereoCrafter step).
The reference has its colour match commented out here (m2s:275, 284), so there is none.  The file gets the blended frames with
--apply_edge_blending, else the pasted ones (m2s:310-329); the pasted ones feed the overlap either way (m2s:308, 332).

The chunk schedule is the reference's (m2s:398-453) and stereo_crafter_infill's, with the same decision for the reference's
off-by-three (m2s:437-440); infill_clip describes it and runs it.  The original frames are carried through the overlap with the others.
"""
from __future__ import annotations

import argparse
import os

from . import _lib
from .clip_io import ClipInputs
from .infill_clip import add_common_flags, callable_from_spec, frames4, infill_chunk, open_clip, run_chunks, run_clips, tuples_from_arguments

IMAGE_W, IMAGE_H = 512, 512               # m2s:215-216
MASK_W, MASK_H = 64, 64                   # m2s:218


def prepare_eye(sbs_color, sbs_mask, org, eye: int, image_size=(IMAGE_W, IMAGE_H), mask_size=(MASK_W, MASK_H)):
    """m2s:224-261 for one eye (0 = left, read mirrored; 1 = right) of uint8 CUDA [N,H,2W,3] colour and infill-mask frames and the
    original frames [N,oh,ow,3] -> (image [N,ih,iw,3], org_image [N,ih,iw,3], mask [N,mh,mw], hole counts int32 [N]), on the device."""
    import torch
    frames4(sbs_color, name="sbs_color"), frames4(sbs_mask, name="sbs_mask", shape=tuple(sbs_color.shape), device=sbs_color)
    frames4(org, name="org", shape=(int(sbs_color.shape[0]), None, None, 3), device=sbs_color)
    if sbs_color.shape[2] % 2:
        raise ValueError(f"sbs_color must hold two eyes side by side, got a width of {int(sbs_color.shape[2])}")
    N, H, W2 = (int(v) for v in sbs_color.shape[:3])
    (iw, ih), (mw, mh) = image_size, mask_size
    dev = sbs_color.device
    image = torch.empty((N, ih, iw, 3), dtype=torch.uint8, device=dev)
    org_image = torch.empty((N, ih, iw, 3), dtype=torch.uint8, device=dev)
    mask = torch.empty((N, mh, mw), dtype=torch.uint8, device=dev)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    _lib.shared_context(dev).call(
        "mdvt_m2svid_prepare_eye", W2 // 2, H, N, int(eye), sbs_color.data_ptr(), sbs_color.stride(1), sbs_color.stride(0),
        sbs_mask.data_ptr(), sbs_mask.stride(1), sbs_mask.stride(0), org.data_ptr(), int(org.shape[2]), int(org.shape[1]), org.stride(1), org.stride(0),
        iw, ih, mw, mh, image.data_ptr(), image.stride(1), image.stride(0), org_image.data_ptr(), org_image.stride(1), org_image.stride(0),
        mask.data_ptr(), mask.stride(1), mask.stride(0), counts.data_ptr(), _lib.stream_arg(dev))
    return image, org_image, mask, counts


def deal_with_frame_chunk(keep_first_three: bool, color, mask, org, keep_last_three: bool, fps: float, generate,
                          image_size=(IMAGE_W, IMAGE_H), mask_size=(MASK_W, MASK_H)):
    """m2s:211-332 on a chunk of uint8 CUDA [T,H,2W,3] colour and mask frames and [T,oh,ow,3] original frames.  Returns (first,
    pasted, blended): the chunk's index of the first frame it writes and the pasted (m2s:303-308) and blended (m2s:312-327) frames
    from there to the last one it writes."""
    return infill_chunk(keep_first_three, keep_last_three, color, mask, lambda eye: prepare_eye(color, mask, org, eye, image_size, mask_size),
                        lambda image, org_image, mmask: generate(image, mmask, org_image, fps))      # (no colour match: m2s:275, 284)


def process_pair(sbs_color_video_path: str, sbs_mask_video_path: str, color_video_path: str, generate, max_frames: int = -1, batch: int = 8,
                 device=None, *, apply_edge_blending: bool = False, video_decoder: str = "host", video_encoder: str = "host",
                 image_size=(IMAGE_W, IMAGE_H), mask_size=(MASK_W, MASK_H)):
    """m2s:367-461.  `.mkv` inputs give `<sbs_color>_infilled.mkv` at the side-by-side colour video's frame rate, frame dumps (`.npy`,
    uint8 [N,H,2W,3] and [N,oh,ow,3]) give `<sbs_color>_infilled.npy`; either is written under its `_tmp_infilled` name and renamed
    once every frame is in.  A mask clip shorter than the colour clip means black masks for the rest (m2s:415-417); an original clip
    shorter than the frames asked for is a ValueError (the reference raises when it gets there, m2s:421-423).  Returns the output path."""
    with ClipInputs() as inp:
        clip = open_clip(inp, sbs_color_video_path, sbs_mask_video_path, [("color_video", color_video_path, False, "org color ended early")],
                         max_frames, video_decoder, video_encoder, device)
        run_chunks(inp, clip, batch, lambda first, last, fps, color, mask, org: deal_with_frame_chunk(first, color, mask, org, last, fps, generate,
                                                                                                   image_size, mask_size),
                   store_blended=apply_edge_blending)              # m2s:310-329
    return clip.final


class M2SVidGenerator:
    """The default generator: the m2svid model with the reference's float conversion and batch layout (m2s:58-114, 485-488).  Needs
    the m2svid checkout with its Hi3D third-party tree, omegaconf and the weights; UNTESTED here (none of them is available to this
    project).  num_inference_steps is accepted for the reference's command line, which sets it and never hands it to the model."""

    def __init__(self, num_inference_steps: int = 5, config_path: str = "m2svid/configs/m2svid.yaml", weights_path: str = "ckpts/m2svid_weights.pt"):
        try:
            import sys
            for sub in ("m2svid", os.path.join("m2svid", "third_party", "Hi3D-Official")):      # m2s:17-18
                if os.path.abspath(sub) not in sys.path:
                    sys.path.append(os.path.abspath(sub))
            from omegaconf import OmegaConf
            from sgm.util import instantiate_from_config
        except ImportError as e:
            raise RuntimeError(f"the m2svid generator needs the m2svid checkout (sgm) and omegaconf ({e}); "
                               "install them or name another model with --generator pkg.module:callable") from None
        config = OmegaConf.load(config_path)
        model = instantiate_from_config(config.model).cpu()
        model.init_from_ckpt(weights_path)
        self.model, self.steps = model.cuda().half().eval(), int(num_inference_steps)

    def __call__(self, frames, masks, org_frames, fps):
        import torch

        def video(t):                                              # [t,h,w,c] u8 -> [1,c,t,h,w] in -1 .. 1 (m2s:62-76, 89-93)
            return (t.permute(0, 3, 1, 2).float() / 255.0 * 2 - 1).permute(1, 0, 2, 3)[None]
        org = video(org_frames)
        batch = {"video": org, "video_2nd_view": org, "reprojected_video": video(frames),
                 "reprojected_mask": (masks.float().unsqueeze(1).permute(1, 0, 2, 3) / 255.0 * 2 - 1)[None],      # m2s:78-85
                 "fps_id": torch.tensor([fps]).cuda(), "caption": [""], "motion_bucket_id": torch.tensor([127]).cuda()}
        with torch.inference_mode():
            out = self.model.generate(batch)["generated-video"]
        out = ((out[0] + 1.0) / 2.0).clip(0, 1).permute(1, 2, 3, 0).float()      # m2s:105
        return (out * 255).to(torch.uint8).to(frames.device).contiguous()        # m2s:114: truncation, like astype(np.uint8)


def load_generator(spec: str, num_inference_steps: int = 5):
    """`m2svid` (the default model) or `pkg.module:callable`."""
    return M2SVidGenerator(num_inference_steps) if spec == "m2svid" else callable_from_spec(spec, "m2svid")


def triples_from_arguments(color_video: str, sbs_color_video: str, sbs_mask_video: str):
    """m2s:494-507: one (sbs_color, sbs_mask, color) triple, or -- if the side-by-side colour argument is a .txt list -- the triples of
    three lists of equal length.  The lists are read and compared before any clip is opened."""
    return tuples_from_arguments([("sbs_color_video", sbs_color_video), ("sbs_mask_video", sbs_mask_video), ("color_video", color_video)])


def build_parser():
    p = argparse.ArgumentParser(description="m2svid infill script (FFV1 .mkv videos, or frame dumps)")
    p.add_argument("--color_video", type=str, required=True, help="Original input video (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--sbs_color_video", type=str, required=True, help="side by side stereo video rendered with point clouds in the masked area, or the matching .txt list")
    p.add_argument("--sbs_mask_video", type=str, required=True, help="side by side stereo video mask, or the matching .txt list")
    p.add_argument("--num_inference_steps", default=5, type=int, help="number of diffusion steps of the m2svid generator. More look better but is slower", required=False)
    p.add_argument("--apply_edge_blending", action="store_true", help="applies blending of the downward facing side of edges to reduce halo effect", required=False)
    p.add_argument("--generator", default="m2svid", type=str,
                   help="not a reference flag: the in-painting model, 'm2svid' (default) or pkg.module:callable with "
                        "generate(frames, masks, org_frames, fps) -> frames on uint8 CUDA tensors [T,512,512,3], [T,64,64] and [T,512,512,3]")
    return add_common_flags(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    kw = dict(batch=args.batch, apply_edge_blending=args.apply_edge_blending, video_decoder=args.video_decoder, video_encoder=args.video_encoder)
    # (the original video is no output of clip.run: it has no per-rank form)
    return run_clips([("sbs_color_video", args.sbs_color_video), ("sbs_mask_video", args.sbs_mask_video), ("color_video", args.color_video)],
                     args.max_frames, lambda paths, generate: process_pair(*paths, generate, args.max_frames, **kw), precheck=(True, True, False),
                     load=lambda: load_generator(args.generator, args.num_inference_steps))


if __name__ == "__main__":
    import sys
    sys.exit(main())
