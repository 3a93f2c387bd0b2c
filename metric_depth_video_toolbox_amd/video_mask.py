"""The host side of the reference's generate_video_mask.py (gvm:), step 3 of movie_2_3D.py: the command line, the file names with
their tmp -> rename step, the frame count of --max_frames, the `--generator` loader and U2-Net's constants.  Plain host logic: no
tensor's address is taken here.  tools/generate_video_mask.py runs the step on the device with these pieces and step_device.py's
wrappers of the three entry points of include/mdvt_video_mask.h.

The step is rembg's remove(only_mask=True) around a U2-Net (gvm:21).  rembg is not available to this project: what it does around the
network is stated in include/mdvt_video_mask.h from its source (sessions/base.py: normalize, sessions/u2net.py: predict), and the
default `rembg_u2net` wrapper below is UNTESTED."""
from __future__ import annotations

import argparse

from .step_clip import add_device_flags, callable_from_spec, clips_from_argument, frames_to_write, output_pair  # noqa: F401 (exported)

# rembg's U2netSession.predict: normalize(img, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), (320, 320)); other rembg models differ in
# these numbers only
U2NET_MEAN = (0.485, 0.456, 0.406)
U2NET_STD = (0.229, 0.224, 0.225)
U2NET_SIZE = 320
DEFAULT_GENERATOR = "rembg_u2net"
DEFAULT_FPS = 30.0                                        # gvm:78: cap.get(cv2.CAP_PROP_FPS) or 30.0


def build_parser():
    """gvm:135-138 under its names, and the flags that are not the reference's."""
    p = argparse.ArgumentParser(description="MDVT mask video generator")
    p.add_argument("--color_video", type=str, required=True, help="the colour video (.mkv, or a .npy frame dump), or a .txt list of them")
    p.add_argument("--max_frames", type=int, default=-1, help="maximum number of frames; -1 = no limit")
    p.add_argument("--batch_size", type=int, default=8, help="micro-batch size: frames per read, per call of the model and per write")
    p.add_argument("--model_size", type=int, default=U2NET_SIZE,
                   help="not a reference flag: the side of the square the frames are resized to for the model (U2-Net: 320)")
    p.add_argument("--generator", default=DEFAULT_GENERATOR, type=str,
                   help=f"not a reference flag: the model, '{DEFAULT_GENERATOR}' (default; needs rembg and onnxruntime) or pkg.module:callable "
                        "with infer(x) -> pred: x float32 CUDA [n,3,S,S], pred float32 CUDA [n,h,w] or [n,1,h,w] (INTEGRATION.md states the contract)")
    return add_device_flags(p)


def check_flags(a):
    """What is refused before any file is opened."""
    if int(a.batch_size) < 1:
        raise ValueError(f"--batch_size must be at least 1, got {a.batch_size}")
    if not 1 <= int(a.model_size) <= 8192:
        raise ValueError(f"--model_size must be 1 .. 8192, got {a.model_size}")
    if int(a.max_frames) < -1:
        raise ValueError(f"--max_frames must be -1 (no limit) or a count, got {a.max_frames}")


def output_paths(color_video: str, video: bool = True):
    """(tmp, final): gvm:66-67; a .npy frame dump gives a .npy mask."""
    return output_pair(color_video, video, "mask")


class RembgU2NetGenerator:
    """rembg's u2net session behind infer(x) -> pred: the network alone, one frame at a time as gvm:32 feeds it (sessions/u2net.py:
    inner_session.run(None, {input name: x}) and [0][:, 0, :, :]).  The tensors cross the host here: onnxruntime takes NumPy arrays.
    UNTESTED: rembg and onnxruntime are not available to this project."""

    def __init__(self):
        import importlib
        try:
            rembg = importlib.import_module("rembg")
            importlib.import_module("onnxruntime")
        except ImportError as e:
            raise RuntimeError(f"the {DEFAULT_GENERATOR} generator needs the rembg and onnxruntime packages ({e}); install them or name "
                               "another model with --generator pkg.module:callable") from None
        self.session = rembg.new_session("u2net").inner_session
        self.input_name = self.session.get_inputs()[0].name

    def __call__(self, x):
        import numpy as np
        import torch
        host = x.cpu().numpy()
        pred = [self.session.run(None, {self.input_name: host[k:k + 1]})[0][:, 0, :, :] for k in range(host.shape[0])]
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(pred), dtype=np.float32)).to(x.device)


def load_generator(spec):
    """`rembg_u2net` (the default model; None too) or `pkg.module:callable`."""
    if spec is None or spec == DEFAULT_GENERATOR:
        return RembgU2NetGenerator()
    return callable_from_spec(spec, DEFAULT_GENERATOR)
