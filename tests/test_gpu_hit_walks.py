"""Every closest-hit walk, ray by ray, on the edge-case rays of tests/hit_ray_cases.py.

rt_hit_rays_walk sends a caller's rays through the walk the render kernels run: the HBM trees
(k_extend, k_finish: closest_hit<F>), k_extend_lds's query (the time-0 tree in LDS, 16-bit stacks,
sign-selected slabs, leafless for one-BVH worlds) and k_camera's (the all-times tree in LDS, or the
time-0 tree when nothing moves).  The truth is the oracle's flat list (hit-obj-list, geometry.scm:33-50,
no tree at all): t must be the same double on every ray.

Found with these rays, and fixed: a ray that lies in a rect's plane (hit_ray_cases.IN_PLANE_RAY).  Its t for
that rect is NaN, the list's order then decides the closest hit, and the library met the world's leaves
grouped by type.  Before the fix, measured on an MI355X, t differed from the list's on 64 and 63 of 1804 rays
(room_mix, room_static) and on 143 of 1792 (curves_small, cornell_bezier alike), all of them in the axis and
plane classes, every walk alike, hit or miss on none; no other ray of any scene or class differed.  Such rays
are now scanned in list order (list_closest, rt_kernels.hip).
"""
import numpy as np
import pytest

import hit_ray_cases as hc
from rtamd import gpu, scenes
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

WALK_NAMES = {hc.WALK_HBM: "hbm", hc.WALK_LDS_TIME0: "lds_time0", hc.WALK_LDS_CAMERA: "lds_camera"}
_runs = {}


def _run(oracle_mod, name):
    """{walk: (classes, rays, class index per ray, t, material, the list's t, the list's material)}, once per scene."""
    if name not in _runs:
        make, classes, walks = hc.CASES[name]
        sc, rays = hc.scene_rays(name, make, classes)
        flat = hc.oracle_flat(oracle_mod, name, make, classes)
        out = {}
        for walk in walks:
            use = [c for c in classes if c in hc.walk_rays(rays, walk)]
            allr = np.concatenate([rays[c][0] for c in use])
            cls_of = np.concatenate([np.full(len(rays[c][0]), i) for i, c in enumerate(use)])
            t, m = gpu.hit_rays(sc, allr, walk=walk)
            out[walk] = (use, allr, cls_of, t, m, np.concatenate([flat[c][0] for c in use]),
                         np.concatenate([flat[c][1] for c in use]))
        _runs[name] = out
    return _runs[name]


def _check(name, walk, run, keep=None):
    """The issue's rule on the rays of mask `keep` (all): t the same double on every ray (two NaNs are equal),
    the same hit / miss on every ray, the material on all but n // 1000 rays (the allowance
    test_hit_rays_vs_oracle_hit_world grants ties in t; t is equal on those as on every ray)."""
    use, allr, cls_of, t, m, et, em = run
    keep = np.ones(len(allr), dtype=bool) if keep is None else keep
    t_bad = ~hc.same_t(t, et) & keep
    hit_bad = ((m >= 0) != (em >= 0)) & keep
    mat_bad = (m != em) & keep
    for i, c in enumerate(use):
        k = (cls_of == i) & keep
        print("%-13s %-10s %-9s %4d rays %4d hits %3d NaN t: t differs on %d, hit/miss on %d, material on %d" % (
            name, WALK_NAMES[walk], c, int(k.sum()), int((em[k] >= 0).sum()), int(np.isnan(et[k]).sum()),
            int(t_bad[k].sum()), int(hit_bad[k].sum()), int(mat_bad[k].sum())))
    show = [(use[cls_of[k]], allr[k].tolist(), (et[k], int(em[k])), (t[k], int(m[k])))
            for k in np.flatnonzero(t_bad | hit_bad | mat_bad)[:4]]
    assert not t_bad.any(), (int(t_bad.sum()), show)
    assert not hit_bad.any(), (int(hit_bad.sum()), show)
    assert int(mat_bad.sum()) <= int(keep.sum()) // 1000, (int(mat_bad.sum()), show)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_walks_vs_flat_list_oracle(sched, oracle_mod, name):
    """Per scene, every walk it supports against the flat-list oracle, on every ray of every class."""
    for walk, run in _run(oracle_mod, name).items():
        _check(name, walk, run)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_walks_vs_oracle_off_the_rect_planes(sched, oracle_mod, name):
    """The same rule on the rays that do not lie in a rect's plane (all of them in scenes without rects): what
    the walks themselves answer — slabs, stacks, t caps, leaf tests — with the order of the list set aside."""
    make, classes, _ = hc.CASES[name]
    P = hc.Prims(hc.scene_rays(name, make, classes)[0])
    for walk, run in _run(oracle_mod, name).items():
        _check(name, walk, run, ~hc.in_rect_plane(P, run[1]))


@pytest.mark.parametrize("name", [n for n, c in hc.CASES.items() if len(c[2]) > 1])
def test_lds_walks_equal_hbm_walk(sched, oracle_mod, name):
    """The LDS walks' t (and material) arrays equal the HBM walk's bit for bit, class by class."""
    runs = _run(oracle_mod, name)
    use0, _, cls0, t0, m0 = runs[hc.WALK_HBM][:5]
    for walk in (hc.WALK_LDS_TIME0, hc.WALK_LDS_CAMERA):
        use, _, cls_of, t, m = runs[walk][:5]
        for i, c in enumerate(use):
            a, b = cls_of == i, cls0 == use0.index(c)
            assert hc.same_t(t[a], t0[b]).all() and np.array_equal(m[a], m0[b]), (WALK_NAMES[walk], c)


@pytest.mark.parametrize("name", ["room_static", "room_mix"])
def test_in_plane_ray_takes_the_lists_order(sched, oracle_mod, name):
    """hit_ray_cases.IN_PLANE_RAY, the regression case of the list-order defect: (NaN, ceiling) by the list,
    whatever the walk (the grouped scan alone gave (6.0, the wall x = -6) on every walk)."""
    make, classes, walks = hc.CASES[name]
    sc, _ = hc.scene_rays(name, make, classes)
    o = oracle_mod.build_scene(sc)
    o.set_bvh_flat(True)
    ray = np.array([hc.IN_PLANE_RAY[0]])
    et, em = hc.oracle_hits(o, ray)
    assert np.isnan(et[0]) and em[0] == 2
    for walk in walks:
        t, m = gpu.hit_rays(sc, ray, walk=walk)
        print(name, WALK_NAMES[walk], (t[0], int(m[0])), "list:", (et[0], int(em[0])))
        assert hc.same_t(t, et).all() and m[0] == em[0], (WALK_NAMES[walk], t[0], int(m[0]))


def test_scene_set_reaches_every_lds_instance(sched):
    """Over the scene set both k_extend_lds instances (SOLO or not) and all four k_camera instances (all-times
    or time-0 tree x SOLO or not) are what rt_hit_rays_walk ran; the 2000-sphere scene and the curve scenes
    have no LDS walk and refuse it."""
    extend, camera = set(), set()
    for name, (make, classes, walks) in hc.CASES.items():
        sc, _ = hc.scene_rays(name, make, classes)
        info = gpu.scene_info(gpu.upload(sc))
        print(name, {k: info[k] for k in ("bvh_solo", "tree0_any_time", "extend_lds_bytes", "camera_lds_bytes")})
        one = np.zeros((1, 7))
        one[0, 3] = 1.0
        if hc.WALK_LDS_TIME0 in walks:
            assert info["extend_lds_bytes"] > 0 and info["camera_lds_bytes"] > 0
            extend.add(bool(info["bvh_solo"]))
            camera.add((not info["tree0_any_time"], bool(info["bvh_solo"])))
        else:
            assert info["extend_lds_bytes"] == 0 and info["camera_lds_bytes"] == 0
            for walk in (hc.WALK_LDS_TIME0, hc.WALK_LDS_CAMERA):
                with pytest.raises(RtError, match="LDS"):
                    gpu.hit_rays(sc, one, walk=walk)
            gpu.hit_rays(sc, one, walk=hc.WALK_HBM)
    assert extend == {False, True}
    assert camera == {(False, False), (False, True), (True, False), (True, True)}


def test_walk_errors_and_block_tails(sched):
    make, classes, _ = hc.CASES["room_mix"]
    sc, rays = hc.scene_rays("room_mix", make, classes)
    allr = np.concatenate([rays[c][0] for c in classes if c != "time"])
    with pytest.raises(RtError, match="unknown walk"):
        gpu.hit_rays(sc, allr[:4], walk=3)
    with pytest.raises(RtError, match="unknown walk"):
        gpu.hit_rays(sc, allr[:4], walk=-1)
    for bad_time in (-0.0, 0.5, float("nan")):
        r = allr[:4].copy()
        r[2, 6] = bad_time
        with pytest.raises(RtError, match=r"time \+0\.0 only \(ray 2"):
            gpu.hit_rays(sc, r, walk=hc.WALK_LDS_TIME0)
        gpu.hit_rays(sc, r[:2], walk=hc.WALK_LDS_TIME0)
    for walk in WALK_NAMES:
        with pytest.raises(RtError, match="media"):
            gpu.hit_rays(scenes.cornell_smoke(16, 16), np.zeros((1, 7)), walk=walk)
        t, m = gpu.hit_rays(sc, np.zeros((0, 7)), walk=walk)
        assert t.shape == (0,) and m.shape == (0,)
        full_t, full_m = gpu.hit_rays(sc, allr, walk=walk)
        for n in (1, 255, 256, 257, 511, 512, 513):     # around a wave multiple and the LDS kernels' block
            t, m = gpu.hit_rays(sc, allr[:n], walk=walk)
            assert hc.same_t(t, full_t[:n]).all() and np.array_equal(m, full_m[:n]), (WALK_NAMES[walk], n)
