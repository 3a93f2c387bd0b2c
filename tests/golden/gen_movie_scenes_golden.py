#!/usr/bin/env python3
"""Generate tests/golden/movie_scenes.json from the reference's own movie_2_3D.split_scenes and plan_scene_files.

Run ONLY where the reference is checked out; MDVT_REFERENCE names its directory.  The reference is imported with cv2 stubbed, as
tests/golden/gen_golden.py does; none of its text travels: the fixture holds the inputs and its functions' outputs.

    MDVT_REFERENCE=<checkout of the reference> python tests/golden/gen_movie_scenes_golden.py
"""
import copy
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MDVT_REFERENCE")

HEADER = ["Scene Number", "Start Frame", "Start Timecode", "Start Time (seconds)", "End Frame", "End Timecode", "End Time (seconds)",
          "Length (frames)", "Length (timecode)", "Length (seconds)"]


def row(k, a, b, fps=24.0, **extra):
    """A list-scenes row of the scene [a, b) (0-based), as the CSV reader hands it over: strings."""
    def tc(s):
        ms = round(s * 1000)
        return "%02d:%02d:%02d.%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)
    d = dict(zip(HEADER, [str(k), str(a + 1), tc(a / fps), "%.3f" % (a / fps), str(b), tc(b / fps), "%.3f" % (b / fps),
                          str(b - a), tc((b - a) / fps), "%.3f" % ((b - a) / fps)]))
    d.update(extra)
    return d


def cases():
    plain = [row(1, 0, 16), row(2, 16, 32), row(3, 32, 40)]
    long = [row(1, 0, 100), row(2, 100, 3200, Engine="vda", Infill="No"), row(3, 3200, 3200), row(4, 3200, 4700, fps=23.976, Convergence="No", Note="kept")]
    columns = [row(1, 0, 30, Engine="", Infill="Yes", Convergence="Yes"), row(2, 30, 90, Engine="depthcrafter", Infill="No", Convergence="No"),
               row(3, 90, 91, Engine="unik3d")]
    return [
        dict(name="plain", scenes=plain, max_scene_frames=1500, end_scene=-1, existing=[]),
        dict(name="long_zero_extra", scenes=long, max_scene_frames=1500, end_scene=-1, existing=[]),
        dict(name="long_end_scene", scenes=long, max_scene_frames=1500, end_scene=3,
             existing=["scene_1.mkv_depth.mkv_stereo.mkv", "scene_2.mkv", "scene_3.mkv_depth.mkv_stereo.mkv_infilled.mkv"]),
        dict(name="exact_multiple", scenes=[row(1, 0, 3000), row(2, 3000, 3001)], max_scene_frames=1500, end_scene=-1, existing=[]),
        dict(name="columns", scenes=columns, max_scene_frames=50, end_scene=-1, existing=["scene_2.mkv_depth.mkv_stereo.mkv_infilled.mkv"]),
    ]


def main():
    if not REF or not os.path.isfile(os.path.join(REF, "movie_2_3D.py")):
        raise SystemExit("set MDVT_REFERENCE to the directory that holds the reference's movie_2_3D.py")
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, REF)
    import movie_2_3D as ref
    out = []
    for case in cases():
        split = ref.split_scenes(copy.deepcopy(case["scenes"]), max_scene_frames=case["max_scene_frames"])
        with tempfile.TemporaryDirectory() as tmp:
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                os.makedirs("out")
                for f in case["existing"]:
                    open(os.path.join("out", f), "w").close()
                planned = ref.plan_scene_files(copy.deepcopy(split), "out", case["end_scene"])
            finally:
                os.chdir(cwd)
        out.append(dict(case, split=split, planned=planned))
    with open(os.path.join(HERE, "movie_scenes.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote movie_scenes.json: {len(out)} cases, {sum(len(c['split']) for c in out)} scenes after the split")


if __name__ == "__main__":
    main()
