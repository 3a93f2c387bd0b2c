"""The host codec as a stand-alone program under the sanitizers: tests/video_host.cpp compiled together with the library's own
sources (csrc_host/*.cpp over csrc/mdvt_ffv1_core.h), run as a child process.  Round trips through both writers and the reader,
and two damaged Matroska files: a TrackEntry that ends inside a child's header (which used to end the process) and a file cut
inside the first SimpleBlock's header."""
import glob
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "metric_depth_video_toolbox_amd")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _build(tmp, flags):
    """-> (program, None), or (None, the compiler's complaint); the translation units are compiled side by side"""
    gxx = [shutil.which("g++"), "-std=c++17", "-O1", "-g", "-pthread"] + flags
    srcs = [os.path.join(REPO, "tests", "video_host.cpp")] + sorted(glob.glob(os.path.join(PKG, "csrc_host", "*.cpp")))
    objs = [os.path.join(tmp, os.path.basename(src) + ".o") for src in srcs]
    jobs = [subprocess.Popen(gxx + ["-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), "-I", os.path.join(PKG, "csrc"), "-c", "-o", obj, src],
                             stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for src, obj in zip(srcs, objs)]
    errors = [j.communicate()[1] for j in jobs]
    if any(j.returncode for j in jobs):
        return None, "".join(errors)[-2000:]
    exe = os.path.join(tmp, "video_host")
    r = subprocess.run(gxx + ["-o", exe] + objs, capture_output=True, text=True)
    return (None, r.stderr[-2000:]) if r.returncode else (exe, None)


def test_round_trips_and_damaged_files_under_the_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = str(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    exe, why = _build(tmp, SANITIZE)
    sanitized = exe is not None and subprocess.run([exe], capture_output=True, env=env).returncode == 2       # (no argument: usage, status 2)
    if not sanitized:                                                      # a compiler without the static runtimes: the plain program
        exe, why = _build(tmp, [])
    assert exe is not None, why
    r = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr[-2000:], "sanitized" if sanitized else "NOT sanitized: the compiler has no static sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert sum(line.startswith("round trip") and line.endswith(": ok") for line in lines) == 6
    cut = [line for line in lines if line.startswith("TrackEntry cut inside a child's header: ")]
    assert len(cut) == 1 and int(cut[0].split(": ")[1].split(",")[0]) < 0 and cut[0].split(", ", 1)[1].strip()
    assert any(line.startswith("file cut inside the first SimpleBlock's header: -3, ") and line.endswith("holds no video frames") for line in lines)
