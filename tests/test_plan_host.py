"""The render scheduler's arithmetic and pool layout without a GPU (nothing preloaded, nothing loaded into python):
tests/csrc/plan_check.cpp sweeps scheme-raytrace_amd/csrc/rt_plan.h (compiled with AddressSanitizer and UBSan)
against the formulas the scheduler had inline before they moved there, and prints the pinned cases asserted here."""
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scheme-raytrace_amd", "csrc")

SECTIONS = ["pool_layout", "plan_render", "tail_paths", "pool_cap_for", "step_slot"]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "csrc", "plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr.strip() == ""
    return json.loads(r.stdout)


def test_sweeps_match_the_inline_formulas_under_sanitizers(plan):
    """pool_layout, plan_render, tail_paths, pool_cap_for and step_slot equal the restated formulas over the grids,
    and the layout's invariants hold (carved arrays disjoint, aligned and inside the pool; scap < 2^32; HitBuf's
    five strides; plan_render's chunk and lane bounds; step_slot's distinct slots).  No sanitizer report."""
    assert sorted(plan) == sorted(SECTIONS)
    for name in SECTIONS:
        assert plan[name]["nfailed"] == 0 and plan[name]["failed"] == [], (name, plan[name]["failed"])


def test_plan_render_pinned_cases(plan):
    """(npix, spp, pool_cap, lanes) -> (chunk, nchunks, nlanes), worked out by hand: test_gpu_production.py's
    8 chunks of 3 passes on 2 lanes; 9 passes, where the even-count step raises 3 chunks to 4 and the ceiling
    brings them back; one pass; a pool smaller than one pass, which still renders one pass per chunk."""
    assert plan["plan_render"]["values"] == [[3, 8, 2], [3, 3, 2], [1, 1, 1], [1, 2, 2]]


def test_tail_paths_pinned_cases(plan):
    """The values of tail_paths' own comment: B/4 for one chunk of 1920x1080, B/64 for two chunks of 4 passes,
    the bounded B/256 of Cornell at 256 spp; curve-kernel scenes keep max(32768, B/256) for any chunk count."""
    assert plan["tail_paths"]["values"] == [518400, 129600, 1048576, 32768, 32768]


def test_pool_cap_pinned_cases(plan):
    """RT_OPT_MAX_PATHS 500 -> 1024; no memory figure -> 384 Mi paths; a 288e9-byte device with 2 lanes ->
    288e9 / 100 * 65 / (2 * 276) = 339 130 434, under the 384 Mi cap.  2^30 free bytes: with 2 lanes 65 % of
    them hold 2^30 / 100 * 65 / 552 = 1 264 369 paths, which is above the floor of 2^20; 4 lanes (632 184 paths)
    reach the floor."""
    assert plan["pool_cap_for"]["values"] == [1024, 384 << 20, 1264369, 1 << 20, 339130434]


def test_plan_is_hip_free():
    txt = open(os.path.join(CSRC, "rt_plan.h")).read()
    assert "hip/" not in txt and "rt_host.h" not in txt and "rt_launch.h" not in txt
    assert set(re.findall(r'#include\s+"([^"]+)"', txt)) == {"rt_device.h"}
    src = open(os.path.join(HERE, "csrc", "plan_check.cpp")).read()
    assert {os.path.basename(i) for i in re.findall(r'#include\s+"([^"]+)"', src)} == {"rt_plan.h"}
