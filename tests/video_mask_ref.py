"""The expected values of the mask-video tests: NumPy restatements of the three entry points of include/mdvt_video_mask.h, written from
the header's text.  lanczos_resize is Pillow's Image.resize(..., LANCZOS) on 8-bit pixels (tests/test_video_mask_cpu.py holds it to
Pillow itself byte for byte, and to tests/golden/video_mask.npz, recorded from Pillow); mask_model_input and mask_from_prediction are
rembg's normalize and the tail of its predict, which that test holds to the literal NumPy expressions of rembg's source."""
import functools
import math

import numpy as np

F = np.float32
PRECISION_BITS = 22
U2NET_MEAN, U2NET_STD, U2NET_SIZE = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), (320, 320)


def _lanczos(t):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
    return sinc(t) * sinc(t / 3) if -3.0 <= t < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def lanczos_table(n_in, n_out):
    """-> (bounds int32 [n_out, 2] = (first sample, taps), k int32 [n_out, ksize]), every step in double as the header writes it."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((n_out, 2), np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = [int(v * (1 << PRECISION_BITS) + (-0.5 if v < 0 else 0.5)) for v in w]       # int(): truncation toward zero
        bounds[xx] = xmin, xmax
        assert 255 * int(np.abs(k[xx].astype(np.int64)).sum()) + (1 << (PRECISION_BITS - 1)) < 1 << 31
    return bounds, k


def _pass(img, n_out, axis):
    """One pass along `axis` of a uint8 array; the other axes are independent."""
    img = np.moveaxis(img, axis, -1)
    n_in = img.shape[-1]
    if n_in == n_out:
        return np.moveaxis(img, -1, axis)
    bounds, k = lanczos_table(n_in, n_out)
    out = np.empty(img.shape[:-1] + (n_out,), np.uint8)
    src = img.astype(np.int64)                                      # (the sums fit an int32: asserted where the table is made)
    for xx in range(n_out):
        a, n = (int(v) for v in bounds[xx])
        ss = (1 << (PRECISION_BITS - 1)) + (src[..., a:a + n] * k[xx, :n].astype(np.int64)).sum(axis=-1)
        out[..., xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def lanczos_resize(img, size, channels):
    """img uint8 [..., H, W] (channels 1: mode L) or [..., H, W, 3] (channels 3); size = (w, h) -> the same with H, W = h, w: the
    horizontal pass first, into uint8, then the vertical pass."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and channels in (1, 3) and (channels == 1 or img.shape[-1] == 3)
    w, h = int(size[0]), int(size[1])
    if channels == 3:
        return _pass(_pass(img, w, -2), h, -3)
    return _pass(_pass(img, w, -1), h, -2)


def mask_model_input(frames, size=U2NET_SIZE, mean=U2NET_MEAN, std=U2NET_STD, bgr=False):
    """frames uint8 [N, H, W, 3] as stored -> float32 [N, 3, h, w], planes R, G, B: rembg's normalize per frame."""
    frames = np.asarray(frames)
    rgb = frames[..., ::-1] if bgr else frames
    out = np.empty((rgb.shape[0], 3, int(size[1]), int(size[0])), F)
    for n, frame in enumerate(rgb):
        im = lanczos_resize(frame, size, 3)
        m = float(im.max()) if im.max() else 1e-6
        for c in range(3):
            out[n, c] = ((im[..., c].astype(np.float64) / m - mean[c]) / std[c]).astype(F)
    return out


def prediction_bytes(pred):
    """float32 [N, h, w] -> uint8 [N, h, w]: (x - mi) / (ma - mi) * 255 in float32, truncated; the header's decrees where that is undefined."""
    pred = np.asarray(pred, F)
    out = np.zeros(pred.shape, np.uint8)
    for n, p in enumerate(pred):
        if not np.isfinite(p).all():
            continue
        mi, ma = p.min(), p.max()
        with np.errstate(over="ignore"):
            rng = F(ma - mi)
        if not (rng > 0) or not np.isfinite(rng):
            continue
        out[n] = np.trunc(F(255.0) * ((p - mi) / rng)).astype(np.uint8)
    return out


def mask_from_prediction(pred, size, channels=1):
    """float32 [N, h, w] -> uint8 [N, H, W] (channels 1) or [N, H, W, 3] at size = (W, H)."""
    m = lanczos_resize(prediction_bytes(pred), size, 1)
    return m if channels == 1 else np.repeat(m[..., None], 3, axis=-1)
