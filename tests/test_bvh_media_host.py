"""Media forests on the host (no GPU, nothing loaded into python but the package): build_scene's forest commit
under AddressSanitizer and UBSan (tests/csrc/bvh_media_check.cpp, its own main beside rt_build.cpp), the C
ABI's announcement, the scenes of tests/bvh_media_cases.py, and the oracle on them, so that the GPU tests'
reference exists."""
import json
import os
import re
import subprocess
import time

import numpy as np
import pytest

import bvh_generic_cases as bc
import bvh_media_cases as mc
from conftest import host_threads
from rtamd import _lib, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scheme-raytrace_amd", "csrc")


@pytest.fixture(scope="module")
def media_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvhm") / "bvh_media_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "csrc", "bvh_media_check.cpp"), os.path.join(CSRC, "rt_build.cpp")])
    return exe


def test_forest_commit_under_sanitizers(media_check):
    """Per scene: every leaf reached by exactly one of its segment's tree or groups, boxes that hold their
    primitives, twins exactly where a sphere moves, order / leaf_pos the list with the media in it, groups as
    [tree] [groups] [medium], rt_tree_info, one digest for 1 and 8 threads; with the threshold out of reach, or
    a Klein set in the scene, the commit without forests; nine qualifying segments get eight trees."""
    r = subprocess.run([media_check], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout)
    forests = {"next_week_small_media": (3, 2, 1), "media_mix": (4, 2, 1), "nine_segments": (9, 8, 0)}
    assert sorted(res) == sorted(list(forests) + [n + "_groups" for n in forests] + ["media_mix_klein"])
    for name, x in res.items():
        assert x["fail"] == [], (name, x["fail"])
        assert x["threads_same"], name
    for name, want in forests.items():
        x = res[name]
        assert (x["segments"], x["trees"], x["twins"]) == want, (name, x)
        assert x["gleaf"] > 0 and x["n_order"] == x["tree_leaves"] + x["group_leaves"] + want[0] - 1
        assert res[name + "_groups"]["n_order"] == 0 and res[name + "_groups"]["gleaf"] == 0
    assert res["media_mix"]["group_leaves"] == 5 and res["nine_segments"]["group_leaves"] == 48
    assert res["media_mix_klein"]["n_order"] == 0 and res["media_mix_klein"]["gleaf"] == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr.strip() == ""


def test_check_program_is_host_code():
    src = open(os.path.join(HERE, "csrc", "bvh_media_check.cpp")).read()
    inc = {os.path.basename(i) for i in re.findall(r'#include\s+"([^"]+)"', src)}
    assert inc == {"rt_build.h"}


def test_abi_announces_media_forests():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt)
    assert re.search(r"#define\s+RT_HAS_MEDIA_BVH\s+1\b", txt)
    assert re.search(r"int\s+rt_hit_rays_stream\s*\(\s*int\s+scene\s*,\s*const\s+double\s*\*\s*rays\s*,\s*int\s+n\s*,\s*"
                     r"uint64_t\s+seed\s*,\s*double\s*\*\s*out_t\s*,\s*int32_t\s*\*\s*out_mat\s*,\s*int32_t\s*\*\s*out_draws\s*\)", txt)
    assert "rt_hit_rays_stream" in _lib.EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "rt_hit_rays_stream" for line in out.splitlines() if line.strip())
    names = [n for n, _ in _lib.RtTreeInfo._fields_]
    assert names[10:12] == ["segments", "segment_trees"]


def test_next_week_media_lists_the_media_where_the_book_does():
    plain, full = scenes.next_week(16, 16, boxes_per_side=2, cluster=3), scenes.SCENES["next_week_media"](
        16, 16, boxes_per_side=2, cluster=3)
    kinds = [o.kind for o in full.obj_list]
    assert [o.kind for o in plain.obj_list] == [k for k in kinds if k != "medium"]
    at = [i for i, k in enumerate(kinds) if k == "medium"]
    assert at == [6, 7]
    glass, blue, mist = full.obj_list[5], full.obj_list[6], full.obj_list[7]
    assert blue.args[0].args[:2] == glass.args[:2] and blue.args[1] == 0.2 and tuple(blue.args[2].args[0]) == (0.2, 0.4, 0.9)
    assert tuple(mist.args[0].args[0]) == (0, 0, 0) and mist.args[0].args[1] == 5000 and mist.args[1] == 0.0001
    assert tuple(mist.args[2].args[0]) == (1, 1, 1)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_scenes_and_rays(name):
    """The segments are what the GPU tests expect, and order_dependent leaves more than half of the rays to the
    comparison of tree and groups commits."""
    sc = mc.CASES[name](mc.NX, mc.NY)
    segs, trees, spheres, generic = mc.EXPECTED[name]
    cut = [[]]
    for o in sc.obj_list:
        if o.kind == "medium":
            cut.append([])
        else:
            cut[-1] += bc.flatten(type(sc)([o], sc.camera, sc.sky_function))
    assert len(cut) == segs
    gen = [sum(1 for lf in s if lf.kind == "r" or lf.chain) for s in cut]
    assert sum(1 for n in gen if n >= bc.GENERIC_MIN) == trees
    assert sum(n for n in gen if n >= bc.GENERIC_MIN) == generic
    assert sum(len(s) - n for s, n in zip(cut, gen) if n >= bc.GENERIC_MIN) == spheres
    rays = mc.scene_rays(name)
    flagged = total = 0
    for c in mc.CLASSES:
        f = mc.order_dependent(sc, rays[c][0])
        print("%-22s %-9s %3d rays, %3d order-dependent" % (name, c, len(f), int(f.sum())))
        flagged += int(f.sum())
        total += len(f)
    assert 0 < flagged < total / 2


@pytest.mark.parametrize("name", list(mc.CASES))
def test_oracle_renders_the_case_scenes_in_seconds(oracle_mod, name):
    """32 x 32 x 4, the GPU test's reference, on the full scene and its thin twin."""
    for thin in (False, True):
        t0 = time.perf_counter()
        acc, segs = oracle_mod.build_scene(mc.CASES[name](32, 32, thin=thin)).render(32, 32, 0, 4, 0x5EED0503,
                                                                                     nthreads=host_threads())
        dt = time.perf_counter() - t0
        print(name, "thin" if thin else "full", "%.2f s, %d segments" % (dt, segs))
        assert np.isfinite(acc).all() and acc.sum() > 0 and segs >= 32 * 32 * 4
        assert dt < 20.0
