"""Writes tests/golden/video_mask.npz: small 8-bit images and what Pillow's Image.resize(..., LANCZOS) makes of them, recorded where
Pillow can be imported, so that tests/test_video_mask_cpu.py holds tests/video_mask_ref.py to Pillow's bytes where it cannot.

    python tests/golden/gen_video_mask_golden.py

Noise and 0/255 steps (the steps drive the filter's negative lobes into both clamps); enlarging, shrinking, one axis each way, a
skipped pass, modes RGB and L.  The file names the Pillow version it was recorded from."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (mode, (in_w, in_h), (out_w, out_h))
CASES = [("RGB", (1, 1), (3, 2)), ("RGB", (5, 4), (16, 12)), ("RGB", (37, 23), (20, 12)), ("RGB", (64, 48), (7, 5)),
         ("RGB", (33, 20), (48, 9)), ("RGB", (40, 25), (40, 11)), ("RGB", (40, 25), (17, 25)), ("RGB", (97, 61), (32, 32)),
         ("L", (32, 32), (1, 1)), ("L", (32, 32), (5, 4)), ("L", (32, 32), (37, 23)), ("L", (32, 32), (100, 7)),
         ("L", (61, 3), (3, 61)), ("L", (50, 40), (21, 13))]


def content(kind, mode, size, seed):
    rng = np.random.default_rng(seed)
    shape = (size[1], size[0]) + ((3,) if mode == "RGB" else ())
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    b = max(1, min(size) // 6)                                     # 0/255 in blocks: edges, whose overshoot reaches both clamps
    cells = rng.integers(0, 2, (-(-size[1] // b), -(-size[0] // b)) + shape[2:]) * 255
    return np.repeat(np.repeat(cells, b, axis=0), b, axis=1)[:size[1], :size[0]].astype(np.uint8)


def main():
    import PIL
    from PIL import Image
    out = {"pillow_version": np.array(PIL.__version__)}
    for k, (mode, src, dst) in enumerate(CASES):
        for kind in ("noise", "step"):
            img = content(kind, mode, src, 1900 + k)
            key = f"{mode}_{src[0]}x{src[1]}_to_{dst[0]}x{dst[1]}_{kind}"
            out[key + "_in"] = img
            out[key + "_out"] = np.asarray(Image.fromarray(img, mode).resize(dst, Image.LANCZOS))
    path = os.path.join(HERE, "video_mask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out) // 2, "images")


if __name__ == "__main__":
    main()
