"""The expected values of the convergence-depth tests: the reference's own lines (find_convergence_depth.py:53-80) run by NumPy on
the test machine, never by the library.  OpenCV's 8-bit COLOR_BGR2GRAY is restated as its integer formula (cv2 is not a dependency);
it is the identity on R = G = B, which is what generate_video_mask.py writes.  Plain module: no fixture, no pytest setting."""
import numpy as np


def gray_of(mask_rgb):
    m = mask_rgb.astype(np.uint32)
    return ((4899 * m[..., 0] + 9617 * m[..., 1] + 1868 * m[..., 2] + 8192) >> 14).astype(np.uint8)


def frame_mean(rgb, mask_rgb=None, max_depth=100):
    """-> (float32 mean or NaN, number of measured pixels) of one RGB depth frame [H, W, 3] under an RGB mask frame, or without one."""
    H, W = rgb.shape[:2]
    depth = np.zeros((H, W), dtype=np.uint32)
    depth_unit = depth.view(np.uint8).reshape((H, W, 4))
    depth_unit[..., 3] = rgb[..., 0]
    depth_unit[..., 2] = rgb[..., 2]
    depth = depth.astype(np.float32) / ((255 ** 4) / max_depth)
    mesured_pixels = depth[gray_of(mask_rgb) > 240] if mask_rgb is not None else depth
    if mesured_pixels.size != 0:
        m = mesured_pixels.mean()
        assert m.dtype == np.float32
        return m, int(mesured_pixels.size)
    return np.float32("nan"), 0


def clip_means(depth, mask=None, max_depth=100):
    """-> (float32 [N], int64 [N]) for RGB depth frames [N, H, W, 3] and the first len(mask) mask frames."""
    n_mask = 0 if mask is None else len(mask)
    res = [frame_mean(depth[k], mask[k] if k < n_mask else None, max_depth) for k in range(len(depth))]
    return np.array([r[0] for r in res], np.float32), np.array([r[1] for r in res], np.int64)


def random_depth(rng, N, H, W, zero_share=0.03):
    """Random R, G and B bytes, some pixels with code 0 (R = B = 0, G anything)."""
    d = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    z = rng.random((N, H, W)) < zero_share
    d[..., 0][z] = 0
    d[..., 2][z] = 0
    return d


def same_bits(got, want):
    """Indices where two float32 arrays differ: equal values, or both NaN, are the same."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
