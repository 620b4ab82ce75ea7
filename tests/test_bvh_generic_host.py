"""Generic tree leaves on the host (no GPU, no commit, nothing preloaded): the world-space leaf boxes and the
tree over them (tests/csrc/bvh_generic_check.cpp: host code with its own main, compiled with AddressSanitizer
and UBSan from the library's own headers), the C ABI's announcement of the feature, and the oracle on the GPU
tests' scenes, so that their reference exists."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_generic_cases as bc
from conftest import host_threads
from rtamd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def generic_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvhg") / "bvh_generic_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "csrc", "bvh_generic_check.cpp")])
    return exe


def test_leaf_boxes_and_threaded_build_under_sanitizers(generic_check):
    """Box-field-like and city-like inputs: every leaf's box holds 1000 surface points of its primitive taken
    through its chain, the 8-thread build equals the serial one bit for bit, primitives that are not finite
    are not tree leaves; no sanitizer report."""
    r = subprocess.run([generic_check], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout)
    assert res["field_leaves"] == 6 * 32 * 32 and res["city_leaves"] > 2048
    assert res["outside_field"] == 0 and res["outside_city"] == 0
    assert res["same_field"] and res["same_city"]
    assert res["refused"] == res["asked"] > 0 and res["finite_ok"]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_check_program_includes_only_the_host_headers():
    src = open(os.path.join(HERE, "csrc", "bvh_generic_check.cpp")).read()
    inc = re.findall(r'#include\s+"([^"]+)"', src)
    assert sorted(os.path.basename(i) for i in inc) == ["rt_bvh.h", "rt_leafbox.h"]
    for h in ("rt_bvh.h", "rt_leafbox.h", "rt_device.h"):
        assert "hip/" not in open(os.path.join(ROOT, "scheme-raytrace_amd", "csrc", h)).read()


def test_abi_announces_the_generic_bvh():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt)
    assert re.search(r"#define\s+RT_HAS_GENERIC_BVH\s+1\b", txt)
    assert re.search(r"int\s+rt_get_tree_info\s*\(\s*int\s+scene\s*,\s*rt_tree_info\s*\*\s*out\s*\)", txt)
    assert "rt_get_tree_info" in _lib.EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "rt_get_tree_info" for line in out.splitlines() if line.strip())
    # the record is ten words and six reserved ones, as the header lays it out
    import ctypes
    assert ctypes.sizeof(_lib.RtTreeInfo) == 64
    m = re.search(r"typedef struct rt_tree_info \{(.*?)\} rt_tree_info;", txt, re.S)
    names = re.findall(r"int32_t\s+([a-z0-9_, ]+?)(?:\[\d+\])?;", m.group(1))
    flat = [n.strip() for group in names for n in group.split(",")]
    assert flat == [n for n, _ in _lib.RtTreeInfo._fields_]


@pytest.mark.parametrize("name", list(bc.CASES) + ["next_week"])
def test_oracle_renders_the_case_scenes(oracle_mod, name):
    """The GPU tests' reference exists: the oracle builds and renders every case scene, and its flat list
    answers the probe rays (hits in every class that hits by construction)."""
    make = bc.next_week_small if name == "next_week" else bc.CASES[name]
    acc, segs = oracle_mod.build_scene(make(16, 16)).render(16, 16, 0, 1, 0x5EED0408, nthreads=host_threads())
    assert np.isfinite(acc).all() and acc.sum() > 0 and segs >= 256
    if name == "next_week":
        return
    sc, rays = bc.scene_rays(name)
    flat = bc.oracle_flat(oracle_mod, name)
    want = bc.expected_tree(sc)
    assert want[1] >= bc.GENERIC_MIN, want                       # the default threshold takes the scene
    for c in bc.CLASSES:
        t, m = flat[c]
        assert len(t) == (12 if c == "nonfinite" else bc.N)
        assert (m >= 0).mean() >= {"nonfinite": 0.0, "inside": 1.0}.get(c, 0.1), (name, c, (m >= 0).mean())
        assert (m >= 0).mean() <= (1.0 if c in ("inside", "aimed", "chained", "nonfinite") else 0.95), (name, c)
    assert np.isnan(flat["chained"][0]).sum() >= 32     # rays in a rect's plane: t = 0/0 by the list
    assert (flat["plane"][1] >= -1).all()


def test_city40_is_past_the_rotation_table():
    full, over = bc.expected_tree(bc.city(16, 16)), bc.expected_tree(bc.city40(16, 16))
    assert full == (2, 241, 0, 13)                   # the ground's empty rotation and 12 angles
    assert over == (2, 1 + 15 * 6, 25 * 6, bc.MAX_ROT)
