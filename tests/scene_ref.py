"""NumPy restatement of scene detection (include/mdvt_scene.h, metric_depth_video_toolbox_amd/scene_detect.py), written apart from
both: OpenCV's 8-bit COLOR_BGR2HSV with H in [0, 180), the difference sums of consecutive frames over the analysed image, the scores,
PySceneDetect's content and adaptive detectors at their 0.6.x defaults, and the list-scenes CSV text."""
import numpy as np

import infill_adapter_ref as iar

_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint((255 << 12) / _I)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint((180 << 12) / (6.0 * _I))]).astype(np.int64)


def hsv_u8(rgb):
    """uint8 [..., 3] in R, G, B order -> int64 (H, S, V) planes."""
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = np.minimum(255, (d * SDIV[v] + 2048) >> 12)
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    hh = (h * HDIV[d] + 2048) >> 12                      # (NumPy's >> on int64 is arithmetic)
    hh = np.where(hh < 0, hh + 180, hh)
    return hh, s, v


def analysed_size(n, factor):
    return int(round(n / factor))                        # Python's round: ties to even


def analysed(frame, factor):
    """The image the sums run over: the frame, or its u8 resize."""
    if factor == 1:
        return frame
    h, w = frame.shape[:2]
    return iar.resize_u8(np.ascontiguousarray(frame), analysed_size(w, factor), analysed_size(h, factor))


def frame_sums(frames, prev=None, factor=1, bgr=False):
    """frames uint8 [n, H, W, 3], prev uint8 [H, W, 3] or None -> [pairs][3] of Python integers: sum |dH|, |dS|, |dV|."""
    seq = ([prev] if prev is not None else []) + [f for f in frames]
    planes = []
    for f in seq:
        f = np.asarray(f)
        planes.append(hsv_u8(analysed(f[..., ::-1] if bgr else f, factor)))
    return [[int(np.abs(a[k] - b[k]).sum()) for k in range(3)] for a, b in zip(planes[:-1], planes[1:])]


def auto_factor(width):
    return 1 if width < 256 else width // 256


def scores(sums, pixels):
    return [float(h + s + v) / float(pixels) / 3.0 for h, s, v in sums]


def content_cuts(sc, threshold=27.0, min_scene_len=15):
    cuts, last = [], 0
    for k in range(1, len(sc) + 1):
        if sc[k - 1] >= threshold and k - last >= min_scene_len:
            cuts.append(k)
            last = k
    return cuts


def adaptive_cuts(sc, adaptive_threshold=3.0, min_content_val=15.0, min_scene_len=15):
    cuts, last, n = [], 0, len(sc) + 1
    for k in range(3, n - 2):
        avg = (sc[k - 3] + sc[k - 2] + sc[k] + sc[k + 1]) / 4.0
        if abs(avg) >= 1e-5:
            ratio = min(sc[k - 1] / avg, 255.0)
        else:
            ratio = 255.0 if sc[k - 1] >= min_content_val else 0.0
        if ratio >= adaptive_threshold and sc[k - 1] >= min_content_val and k - last >= min_scene_len:
            cuts.append(k)
            last = k
    return cuts


def scenes(cuts, n):
    e = [0] + list(cuts) + [n]
    return [(e[i], e[i + 1]) for i in range(len(e) - 1)]


def tc(seconds):
    ms = round(seconds * 1000)
    return "%02d:%02d:%02d.%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)


HEADER = ("Scene Number,Start Frame,Start Timecode,Start Time (seconds),End Frame,End Timecode,End Time (seconds),"
          "Length (frames),Length (timecode),Length (seconds)")


def csv_text(scene_list, fps):
    lines = [",".join(["Timecode List:"] + [tc(a / fps) for a, _ in scene_list[1:]]), HEADER]
    for k, (a, b) in enumerate(scene_list, 1):
        lines.append(",".join([str(k), str(a + 1), tc(a / fps), "%.3f" % (a / fps), str(b), tc(b / fps), "%.3f" % (b / fps),
                               str(b - a), tc((b - a) / fps), "%.3f" % ((b - a) / fps)]))
    return "\n".join(lines) + "\n"


def clip_csv(frames, fps, detector="adaptive", downscale="auto"):
    """The CSV text of a clip uint8 [n, H, W, 3] (R, G, B) at the detectors' defaults."""
    n, h, w = frames.shape[:3]
    factor = auto_factor(w) if downscale == "auto" else int(downscale)
    sc = scores(frame_sums(frames, factor=factor), analysed_size(w, factor) * analysed_size(h, factor))
    cuts = content_cuts(sc) if detector == "content" else adaptive_cuts(sc)
    return csv_text(scenes(cuts, n), fps)


def three_shot_clip(n=40, h=32, w=48, cuts=(16, 32), seed=5):
    """Three synthetic shots: noise around three different colours, cuts in front of frames 16 and 32."""
    rng = np.random.default_rng(seed)
    base = np.array([[235, 200, 30], [30, 180, 60], [40, 60, 210]], np.int64)        # (hues away from 0: noise does not wrap them)
    shot = np.searchsorted(np.array(cuts), np.arange(n), side="right")
    noise = rng.integers(-6, 7, (n, h, w, 3))
    return np.clip(base[shot][:, None, None, :] + noise, 0, 255).astype(np.uint8)
