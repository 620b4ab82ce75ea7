"""Light lists on the host (include/rt.h, "light lists"): rtamd.lights, the NumPy restatement of the rule,
pinned to the oracle for the two lights the oracle knows, checked against itself (two triangles are the rect,
a mixed list is a density, the sampler's draws and picks), the Python refusals, and the HIP-free scene build
with a light list (tests/csrc/lights_check.cpp, compiled beside rt_build.cpp under AddressSanitizer and UBSan)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import light_cases as lc
from rtamd import lights, mesh, scenes
from rtamd import scene as g
from rtamd.camera import make_camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scheme-raytrace_amd", "csrc")


def _uniform_dirs(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------- 1. pinned to the oracle
def _pin(oracle_mod, scene, light, origins, aim):
    """20 000 directions from several origins, half aimed at the light (aim(rng, n) -> points on it)."""
    o_scene = oracle_mod.build_scene(scene)
    rs = np.random.default_rng(7)
    per = 20000 // len(origins)
    bad = total = hits = nans = 0
    for o in origins:
        d = _uniform_dirs(per, rs.integers(1 << 30)) * rs.uniform(0.5, 3.0, size=(per, 1))
        d[: per // 2] = aim(rs, per // 2) - np.array(o)
        got = lights.pdf_value([light], o, d)
        want = np.array([o_scene.light_pdf_value(tuple(o), tuple(v)) for v in d])
        bad += int((~_same_bits(got, want)).sum())
        total += per
        hits += int((want > 0).sum())
        nans += int(np.isnan(want).sum())
    return bad, total, hits, nans


def test_rect_density_is_the_oracles_bit_for_bit(oracle_mod):
    sc = scenes.cornell_mixture(16, 16)

    def aim(rs, n):
        return np.stack([rs.uniform(200, 356, n), np.full(n, 554.0), rs.uniform(215, 345, n)], axis=1)
    origins = [(278.0, 100.0, 278.0), (10.0, 500.0, 30.0), (500.0, 553.0, 278.0), (278.0, 554.0, 278.0), (300.0, 600.0, 250.0)]
    bad, total, hits, nans = _pin(oracle_mod, sc, sc.light, origins, aim)
    print("rect: %d of %d values differ; %d hits" % (bad, total, hits))
    assert total == 20000 and hits > 5000 and bad == 0


def test_sphere_density_is_the_oracles_bit_for_bit_inside_too(oracle_mod):
    sc = lc.sphere_scene()

    def aim(rs, n):
        d = rs.normal(size=(n, 3))
        return np.array([0.0, 3.0, 0.0]) + d / np.linalg.norm(d, axis=1, keepdims=True) * rs.uniform(0, 0.9, size=(n, 1))
    origins = [(0.3, 0.5, 0.2), (5.0, 3.0, -2.0), (0.0, 10.0, 0.0), (0.1, 3.2, 0.1), (0.0, 3.0, 0.3)]   # the last two: inside
    bad, total, hits, nans = _pin(oracle_mod, sc, sc.light, origins, aim)
    print("sphere: %d of %d values differ; %d hits, %d NaN (origins inside)" % (bad, total, hits, nans))
    assert total == 20000 and hits > 5000 and nans > 1000 and bad == 0


# ------------------------------------------------------ 2. two triangles are the rect
def test_two_triangles_are_the_rect():
    n = 200000
    rs = np.random.default_rng(11)
    o = rs.uniform(0, 1, size=(n, 3)) * np.array([555.0, 540.0, 555.0])
    aim = np.stack([rs.uniform(180, 380, n), np.full(n, 554.0), rs.uniform(190, 370, n)], axis=1)
    v = aim - o
    tri = lights.pdf_value(lc.lamp_triangles(), o, v)
    rect = lights.pdf_value([lc.lamp_rect()], o, v)
    hit_t, hit_r = tri > 0, rect > 0
    both = hit_t & hit_r
    rel = np.abs(tri[both] - rect[both]) / rect[both]
    print("two triangles vs the rect: %d rays, %d hit, %d hit/miss disagreements, largest difference %.2f ulps"
          % (n, both.sum(), int((hit_t != hit_r).sum()), rel.max() / 2.0 ** -52))
    assert both.sum() > n // 5 and (~hit_r).sum() > n // 5
    assert np.array_equal(hit_t, hit_r)
    assert rel.max() <= 64 * 2.0 ** -52                          # 64 ulps = 1.42e-14 relative


# ---------------------------------------------------- 3. a mixed list integrates to 1
def test_mixed_list_integrates_to_one():
    lst = lc.lamp_triangles() + [g.make_sphere((190, 90, 190), 90, g.make_lambertian(g.constant_texture((1, 1, 1))))]
    n = 10 ** 6
    vals = lights.pdf_value(lst, (278.0, 100.0, 278.0), _uniform_dirs(n, 3)) * (4 * math.pi)
    est, se = vals.mean(), vals.std(ddof=1) / math.sqrt(n)
    print("mixed list: integral %.5f, se %.5f" % (est, se))
    assert se <= 0.01 and abs(est - 1.0) <= 4 * se


# ------------------------------------------------------------------- 4. random
def test_random_draws_and_samples_land_on_their_lights():
    rect, sphere, (t0, t1) = lc.lamp_rect(), lc.sphere_light(), lc.lamp_triangles()
    o = (278.0, 100.0, 278.0)
    for lst, base in (([rect], 2), ([t0], 2), ([sphere], 6)):
        assert lights.random(lst, o, lc.SEED, 5)[1] == base                     # m == 1: no choice draw
    # 100 000 samples of the rect and 100 000 of the two-triangle list, each held to 99.9 % on its own (so each
    # surface kind is checked, and the list's pick with the triangles)
    n = 200000 // 2
    for lst in ([rect], [t0, t1]):
        dirs = np.array([lights.random(lst, o, lc.SEED, k)[0] for k in range(n)])
        pos = lights.pdf_value(lst, o, dirs) > 0
        print("samples with a positive density: %.4f %%" % (100.0 * pos.mean()))
        assert pos.mean() >= 0.999
    # Four lights that no direction from o meets two of (the diagonal of t0 / t1 apart): which one a sample was
    # taken from is read off the sampled direction itself: the rect or triangle whose own density is positive
    # there, the sphere otherwise (its sampler's three evaluations need not land on it, Q29).
    wall = g.make_xy_rect(50, 150, 200, 300, 500, lc._emit())
    four = [wall, t0, sphere, t1]
    per = np.array([2, 2, 6, 2])
    N = 20000
    got = [lights.random(four, o, lc.SEED, k) for k in range(N)]
    dirs = np.array([d for d, _ in got])
    draws = np.array([c for _, c in got])
    on = np.array([lights.pdf_value([L], o, dirs) > 0 for L in four])           # (4, N)
    on[3] &= ~on[1]                                                              # a sample on the shared diagonal: t0's
    flat_on = on[[0, 1, 3]]
    assert (flat_on.sum(axis=0) <= 1).all()
    picked = np.where(flat_on.any(axis=0), np.array([0, 1, 3])[np.argmax(flat_on, axis=0)], 2)
    counts = np.bincount(picked, minlength=4)
    print("picks over four lights, read from the sampled directions:", counts.tolist(),
          "sphere samples that meet the sphere: %d of %d" % (int(on[2][picked == 2].sum()), int(counts[2])))
    assert (np.abs(counts - N / 4) <= 5 * math.sqrt(3 * N / 16)).all()
    assert (draws == 1 + per[picked]).all()                                      # the choice draw, then the light's own
    assert on[2][picked == 2].mean() > 0.5


# ------------------------------------------------------------- 5. Python refusals
def test_make_scene_refuses_what_the_abi_refuses():
    lam = g.make_lambertian(g.constant_texture((0.5, 0.5, 0.5)))
    cam = make_camera((0, 1, 5), (0, 1, 0), (0, 1, 0), 40, 1, 0, 1, 0, 1)
    sph = g.make_sphere((0, 1, 0), 1, lam)
    # (an empty list is refused too: the keyword's "no light list" is None; n == 0 turning sampling off is the ABI's)
    for bad in ([g.make_box((0, 0, 0), (1, 1, 1), lam)], [g.translate(sph, (1, 0, 0))], [g.rotate_y(sph, 10)],
                [g.make_moving_sphere((0, 0, 0), (0, 1, 0), 0, 1, 1, lam)], [g.make_bvh_node([sph], 0, 1)],
                [sph, g.make_box((0, 0, 0), (1, 1, 1), lam)], []):
        with pytest.raises(ValueError):
            g.make_scene([sph], cam, g.black, lights=bad)
    with pytest.raises(ValueError, match="not both"):
        g.make_scene([sph], cam, g.black, light=sph, lights=[sph])
    sc = g.make_scene([sph], cam, g.black, lights=[g.flip_normals(sph), g.make_mesh(*mesh.icosphere(0), lam)])
    assert len(lights.flatten(sc.lights)) == 21 and sc.light is None
    assert g.make_scene([sph], cam, g.black).lights is None
    ml = scenes.SCENES["cornell_mesh_lights"](16, 16)
    assert [L[0] for L in lights.flatten(ml.lights)] == ["tri", "tri"] and ml.lights[0] is ml.obj_list[2]


def test_the_oracle_is_not_handed_a_light_list(oracle_mod):
    with pytest.raises(NotImplementedError, match="light lists are not restated"):
        oracle_mod.build_scene(lc.room(lights=lc.lamp_halves()))


# --------------------------------------------------- 6. the scene build, sanitized
@pytest.fixture(scope="module")
def lights_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lights") / "lights_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "csrc", "lights_check.cpp"), os.path.join(CSRC, "rt_build.cpp")])
    return exe


def test_scene_build_with_a_light_list_under_sanitizers(lights_check):
    r = subprocess.run([lights_check], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout)
    assert res["order_error"] == "" and res["types"] == "12444412" and res["list_type"] and res["values"]
    assert res["tri_area_nu"] and res["mesh_area"] and res["same_again"] and res["tri_flag"]
    assert res["one_rect"] and res["one_sphere"] and res["one_tri"] and res["off"]
    assert res["cap_4096"] and "RT_MAX_LIGHTS" in res["cap_4097"]
    for key in ("box", "moving_sphere", "translate", "rotate_y", "bvh", "curve", "medium", "klein"):
        assert "a light must be a rect, a sphere or a triangle" in res[key], (key, res[key])
    assert "invalid object id" in res["bad_id"] and "invalid object id" in res["negative_id"]
    assert "holds no light" in res["empty"] and "too deep" in res["flip_cycle"]
    assert res["null_objs"] and res["negative_n"] and res["zero_n"]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr.strip() == ""
