"""Host side of scene detection (step 0 of the reference's movie_2_3D.py, m23d:209-222, which runs PySceneDetect's
`scenedetect -i movie list-scenes`): the integer sums of include/mdvt_scene.h's entry point to scores, cuts, a scene list and
PySceneDetect's `<video stem>-Scenes.csv`.  Importable without torch; no tensor's address is taken here (the device wrapper is
step_device.frame_sums).

PySceneDetect is not observed by this project: what follows restates its 0.6.x defaults from its documentation and is a DECREE of
this project (README, DESIGN.md "Scene detection"), not a measured equality.  All arithmetic is float64.

    score_k  = (sH + sS + sV) / float(pixels) / 3.0        of the pair (k - 1, k): the content detector's weights 1, 1, 1, 0
    content  : a cut in front of frame k when score_k >= threshold (27.0) and k - last_cut >= min_scene_len (15; last_cut starts at 0)
    adaptive : window_width 2; frame k needs two scored frames on each side; avg = the mean of those four scores;
               ratio = min(score / avg, 255) where |avg| >= 1e-5, 255 where |avg| < 1e-5 and score >= min_content_val, else 0;
               a cut in front of k when ratio >= adaptive_threshold (3.0), score >= min_content_val (15.0) and the same
               min_scene_len rule
"""
from __future__ import annotations

import argparse
import csv
import io
import os

DETECTORS = ("adaptive", "content")
THRESHOLD = 27.0
ADAPTIVE_THRESHOLD = 3.0
MIN_CONTENT_VAL = 15.0
MIN_SCENE_LEN = 15
WINDOW_WIDTH = 2
CSV_HEADER = ["Scene Number", "Start Frame", "Start Timecode", "Start Time (seconds)", "End Frame", "End Timecode", "End Time (seconds)",
              "Length (frames)", "Length (timecode)", "Length (seconds)"]
SCENE_FILE_SUFFIX = "-Scenes.csv"                       # m23d:217-218


def round_half_even_div(n: int, factor: int) -> int:
    """Python's round(n / factor) in integers: the header's rule for the analysed image's size."""
    q, r = divmod(int(n), int(factor))
    return q + 1 if 2 * r > factor else (q + (q & 1) if 2 * r == factor else q)


def auto_downscale(width: int) -> int:
    """`--downscale auto`: PySceneDetect's factor for a frame of this width."""
    return 1 if int(width) < 256 else int(width) // 256


def downscale_factor(downscale, width: int, height: int) -> int:
    """The integer factor of --downscale (`auto` or N >= 1); ValueError where it leaves no image."""
    factor = auto_downscale(width) if str(downscale) == "auto" else int(downscale)
    if factor < 1:
        raise ValueError(f"--downscale must be 'auto' or an integer >= 1, got {downscale!r}")
    if round_half_even_div(width, factor) < 1 or round_half_even_div(height, factor) < 1:
        raise ValueError(f"--downscale {factor} leaves no image of a {width}x{height} frame")
    return factor


def analysed_pixels(width: int, height: int, factor: int) -> int:
    return round_half_even_div(width, factor) * round_half_even_div(height, factor)


def scores_from_sums(sums, pixels: int):
    """[(sH, sS, sV)] of the pairs (k - 1, k), k = 1 .. n - 1 -> [score_1 .. score_{n-1}] as Python floats."""
    return [(int(h) + int(s) + int(v)) / float(pixels) / 3.0 for h, s, v in sums]


def content_cuts(scores, threshold: float = THRESHOLD, min_scene_len: int = MIN_SCENE_LEN):
    """scores[k - 1] is frame k's -> the frames a cut stands in front of."""
    cuts, last = [], 0
    for k, score in enumerate(scores, start=1):
        if score >= threshold and k - last >= min_scene_len:
            cuts.append(k)
            last = k
    return cuts


def adaptive_cuts(scores, adaptive_threshold: float = ADAPTIVE_THRESHOLD, min_content_val: float = MIN_CONTENT_VAL,
                  min_scene_len: int = MIN_SCENE_LEN, window_width: int = WINDOW_WIDTH):
    """scores[k - 1] is frame k's -> the frames a cut stands in front of (frame 0 has no score)."""
    cuts, last, w = [], 0, int(window_width)
    n = len(scores) + 1                                  # frames
    for k in range(1 + w, n - w):
        score = scores[k - 1]
        near = [scores[j - 1] for j in range(k - w, k + w + 1) if j != k]
        avg = sum(near) / (2.0 * w)
        if abs(avg) >= 1e-5:
            ratio = min(score / avg, 255.0)
        else:
            ratio = 255.0 if score >= min_content_val else 0.0
        if ratio >= adaptive_threshold and score >= min_content_val and k - last >= min_scene_len:
            cuts.append(k)
            last = k
    return cuts


def detect_cuts(scores, detector: str = "adaptive", threshold: float = THRESHOLD, adaptive_threshold: float = ADAPTIVE_THRESHOLD,
                min_content_val: float = MIN_CONTENT_VAL, min_scene_len: int = MIN_SCENE_LEN):
    if detector == "content":
        return content_cuts(scores, threshold, min_scene_len)
    if detector == "adaptive":
        return adaptive_cuts(scores, adaptive_threshold, min_content_val, min_scene_len)
    raise ValueError(f"--detector must be one of {DETECTORS}, got {detector!r}")


def scenes_from_cuts(cuts, n_frames: int):
    """[(first frame, frame behind the last)] (0-based) of the runs between the cuts; a clip without a cut is one scene."""
    edges = [0] + [int(c) for c in cuts] + [int(n_frames)]
    return list(zip(edges[:-1], edges[1:]))


def timecode(seconds: float) -> str:
    ms = round(seconds * 1000)
    s, ms = divmod(ms, 1000)
    m, s = divmod(s, 60)
    h, m = divmod(m, 60)
    return f"{h:02d}:{m:02d}:{s:02d}.{ms:03d}"


def scene_rows(scenes, fps: float):
    """The CSV's rows as dicts of strings: Start Frame 1-based, End Frame inclusive; a scene [a, b) starts at a / fps, ends at
    b / fps and lasts (b - a) / fps seconds."""
    rows = []
    for k, (a, b) in enumerate(scenes, start=1):
        t0, t1, dt = a / fps, b / fps, (b - a) / fps
        rows.append(dict(zip(CSV_HEADER, [str(k), str(a + 1), timecode(t0), f"{t0:.3f}", str(b), timecode(t1), f"{t1:.3f}",
                                          str(b - a), timecode(dt), f"{dt:.3f}"])))
    return rows


def scene_csv_text(scenes, fps: float, delimiter: str = ",") -> str:
    """PySceneDetect's list-scenes file: `Timecode List:` and the cut timecodes, the header, one row per scene; lines end in \\n."""
    out = io.StringIO()
    w = csv.writer(out, delimiter=delimiter, lineterminator="\n")
    w.writerow(["Timecode List:"] + [timecode(a / fps) for a, _ in scenes[1:]])
    w.writerow(CSV_HEADER)
    for row in scene_rows(scenes, fps):
        w.writerow([row[h] for h in CSV_HEADER])
    return out.getvalue()


def write_scene_csv(path: str, scenes, fps: float, delimiter: str = ",") -> str:
    """Writes the file under a temporary name and renames it -> path."""
    tmp = path + ".tmp"
    with open(tmp, "w", newline="") as fh:
        fh.write(scene_csv_text(scenes, fps, delimiter))
    os.replace(tmp, path)
    return path


def load_scene_csv(path: str, delimiter: str = ","):
    """m23d:233-241: the first row is skipped, the rest is read by DictReader -> [dict of strings]."""
    with open(path, newline="") as fh:
        next(csv.reader(fh))
        return [dict(row) for row in csv.DictReader(fh, delimiter=delimiter)]


def scenes_of_rows(rows):
    """[(first frame, frame behind the last)] of loaded rows: the inverse of scene_rows."""
    return [(int(r["Start Frame"]) - 1, int(r["End Frame"])) for r in rows]


def scene_file_path(color_video: str, output_dir: str = "") -> str:
    """`<video stem>-Scenes.csv` (m23d:217-219), in output_dir where one is given."""
    return os.path.join(output_dir, os.path.splitext(os.path.basename(color_video))[0] + SCENE_FILE_SUFFIX)


def check_flags(args):
    if args.detector not in DETECTORS:
        raise ValueError(f"--detector must be one of {DETECTORS}, got {args.detector!r}")
    if int(args.min_scene_len) < 0:
        raise ValueError("--min_scene_len must be >= 0")
    if int(args.batch) < 1:
        raise ValueError("--batch must be >= 1")
    if str(args.downscale) != "auto" and int(args.downscale) < 1:
        raise ValueError(f"--downscale must be 'auto' or an integer >= 1, got {args.downscale!r}")
    if args.fps is not None and not (float(args.fps) > 0):
        raise ValueError("--fps must be > 0")


def build_parser():
    from .clip_io import VIDEO_DECODERS
    p = argparse.ArgumentParser(description="Lists the scenes of a video as PySceneDetect's list-scenes does (restated defaults of "
                                            "0.6.x); the frame differences are summed on the GPU.")
    p.add_argument("--color_video", type=str, required=True, help="video to analyse (.mkv with FFV1, or a .npy frame dump)")
    p.add_argument("--detector", default="adaptive", choices=DETECTORS, help="detect-adaptive (what a bare list-scenes runs) or detect-content")
    p.add_argument("--threshold", default=THRESHOLD, type=float, help="content detector: the score a cut needs")
    p.add_argument("--adaptive_threshold", default=ADAPTIVE_THRESHOLD, type=float, help="adaptive detector: the ratio a cut needs")
    p.add_argument("--min_content_val", default=MIN_CONTENT_VAL, type=float, help="adaptive detector: the score a cut needs")
    p.add_argument("--min_scene_len", default=MIN_SCENE_LEN, type=int, help="frames between two cuts")
    p.add_argument("--downscale", default="auto", help="'auto' (1 below 256 columns, else width // 256) or an integer factor")
    p.add_argument("--fps", default=None, type=float, help="frame rate of a .npy dump, or of a video that states none (default 30)")
    p.add_argument("--batch", default=64, type=int, help="frames per device call")
    p.add_argument("--video_decoder", choices=VIDEO_DECODERS, default="host",
                   help="where an .mkv input is FFV1-decoded -- 'host' (default), 'device' or 'device_all'")
    p.add_argument("--output", default=None, type=str, help="the CSV to write (default: <video stem>-Scenes.csv beside the video)")
    return p
