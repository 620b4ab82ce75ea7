"""The host half of a scene commit without a GPU (nothing preloaded, nothing loaded into python):
tests/csrc/commit_check.cpp fills scene descriptions directly, runs build_scene (rt_build.cpp, compiled beside
it with AddressSanitizer and UBSan) and checks its decisions against brute force of its own."""
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scheme-raytrace_amd", "csrc")

SCENES = ["a", "b_shared", "b_zero_den", "c", "d", "e", "f", "g"]
ERRORS = {
    "nested": "constant media cannot be nested",
    "curve_boundary": "a constant medium's boundary may hold spheres, rects, boxes and instances only",
    "depth5": "instance nesting deeper than 4 transforms",
    "cycle": "object graph too deep (cycle?)",
    "no_camera": "rt_scene_commit: no camera set (rt_set_camera)",
    "noise": "rt_scene_commit: noise/marble texture needs rt_set_perlin_tables",
}


@pytest.fixture(scope="module")
def commit_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("commit") / "commit_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "csrc", "commit_check.cpp"), os.path.join(CSRC, "rt_build.cpp")])
    return exe


def test_build_scene_decisions_under_sanitizers(commit_check):
    """Scenes (a)-(g): leaf ids, list order, tree leaves and their boxes, time-0 centres, group tiling, flags
    and rt_tree_info as the flattened list implies them; 1 and 8 threads give one digest; (h): the failures
    keep the commit's texts.  No sanitizer report."""
    r = subprocess.run([commit_check], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout)
    assert sorted(res) == sorted(SCENES + list(ERRORS))
    for name in SCENES:
        assert res[name]["failed"] == [], (name, res[name]["failed"])
        assert int(res[name]["digest"], 16) != 0
    for name, text in ERRORS.items():
        assert res[name]["failed"] == [] and res[name]["text"] == text, (name, res[name])
    assert len({res[n]["digest"] for n in SCENES}) == len(SCENES)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr.strip() == ""


def test_scene_build_is_hip_free():
    for h in ("rt_build.cpp", "rt_build.h", "rt_model.h"):
        txt = open(os.path.join(CSRC, h)).read()
        assert "hip/" not in txt and "rt_host.h" not in txt and "rt_launch.h" not in txt, h
    inc = set(re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, "rt_build.cpp")).read()))
    inc |= set(re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, "rt_build.h")).read()))
    assert inc == {"rt_build.h", "rt_model.h", "rt_device.h", "rt_bvh.h", "rt_leafbox.h"}
    src = open(os.path.join(HERE, "csrc", "commit_check.cpp")).read()
    mine = {os.path.basename(i) for i in re.findall(r'#include\s+"([^"]+)"', src)}
    assert "rt_build.h" in mine and mine <= {"rt_build.h", "rt_model.h", "rt_bvh.h", "rt_leafbox.h"}
