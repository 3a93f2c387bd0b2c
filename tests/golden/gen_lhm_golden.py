"""Writes tests/golden/lhm_transfer_*.npz: inputs and outputs of the reference's transfer_lhm_video_refmask (infill_common.py),
run on the build machine only:

    python tests/golden/gen_lhm_golden.py /path/to/the/reference/checkout

Each fixture holds video, reference, mask (uint8), out_f32 and out_f64 (the function's output with single_precision True and False)
and pre_f64, the float64 values the single_precision=False run hands to np.round (captured from the function itself: its module's
`np` is wrapped for the duration of the call).  Inputs come from seeded generators; nothing of the reference is stored but results."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class _NumpyTap:
    """numpy, except that round() remembers what it was given."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(np, name)

    def round(self, a, *args, **kw):
        self.seen.append(np.array(a, copy=True))
        return np.round(a, *args, **kw)


def run_reference(ic, video, reference, mask):
    out32 = ic.transfer_lhm_video_refmask(video, reference, mask, single_precision=True)
    tap = _NumpyTap()
    ic.np = tap
    try:
        out64 = ic.transfer_lhm_video_refmask(video, reference, mask, single_precision=False)
    finally:
        ic.np = np
    T, H, W, C = video.shape
    pre = np.array(tap.seen, dtype=np.float64).reshape(T, H, W, C)
    assert np.array_equal(np.clip(np.round(pre), 0, 255).astype(np.uint8), out64)
    return out32, out64, pre


def structured(rng, T, H, W):
    """A reference video (ramps, a moving disc, some noise), the 'generated' video (a colour cast, gain and noise on top) and a block
    mask (255 = not counted) that moves with the frame."""
    y, x = np.mgrid[0:H, 0:W]
    ref = np.empty((T, H, W, 3), dtype=np.uint8)
    mask = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        base = np.stack([40 + 180 * x / max(W - 1, 1), 30 + 200 * y / max(H - 1, 1), 128 + 90 * np.sin((x + 2 * y + 5 * t) / 9.0)], axis=-1)
        disc = ((x - W * (0.3 + 0.1 * t)) ** 2 + (y - H * 0.5) ** 2) < (min(H, W) * 0.2) ** 2
        base[disc] = base[disc] * 0.4 + np.array([200.0, 60.0, 20.0]) * 0.6
        ref[t] = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        y0, x0 = (H // 4 + t) % max(H // 2, 1), (W // 3 + 2 * t) % max(W // 2, 1)
        mask[t, y0:y0 + max(H // 3, 1), x0:x0 + max(W // 4, 1)] = 255
    gain = np.array([0.8, 1.1, 0.9])
    cast = np.array([18.0, -12.0, 25.0])
    video = np.clip(ref.astype(np.float64) * gain + cast + rng.normal(0, 9, ref.shape), 0, 255).astype(np.uint8)
    return video, ref, mask


def cases():
    rng = np.random.default_rng(20261)
    yield "48x64", structured(rng, 4, 48, 64)
    v, r, m = structured(rng, 3, 5, 7)
    yield "5x7", (v, r, m)
    v, r, m = structured(rng, 2, 12, 16)
    v[0] = np.array([90, 140, 30], dtype=np.uint8)                 # a constant video frame: its covariance is eps on the diagonal
    yield "constant", (v, r, m)
    v, r, m = structured(rng, 3, 12, 16)
    m[0] = 255                                                     # keeps 0, 2 and 3 pixels: the first two fall back to all pixels
    m[1] = 255
    m[1, 3, 4] = m[1, 7, 9] = 0
    m[2] = 255
    m[2, 0, 0] = m[2, 5, 5] = m[2, 11, 15] = 0
    yield "few_kept", (v, r, m)
    # one pair at the model's size does not fit a committed file (its float64 values alone are 18 MB): a 96 x 128 crop of it
    v, r, m = structured(rng, 1, 768, 1024)
    crop = (slice(None), slice(300, 396), slice(420, 548))
    yield "crop96x128", (np.ascontiguousarray(v[crop]), np.ascontiguousarray(r[crop]), np.ascontiguousarray(m[crop]))


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, argv[1])
    import infill_common as ic
    for name, (video, reference, mask) in cases():
        out32, out64, pre = run_reference(ic, video, reference, mask)
        path = os.path.join(HERE, f"lhm_transfer_{name}.npz")
        np.savez_compressed(path, video=video, reference=reference, mask=mask, out_f32=out32, out_f64=out64, pre_f64=pre)
        size = os.path.getsize(path)
        assert size < (1 << 20), f"{path}: {size} bytes"
        print(f"{path}: {size} bytes, {int((out32 != out64).sum())} of {out64.size} values differ between the two precisions")


if __name__ == "__main__":
    main(sys.argv)
