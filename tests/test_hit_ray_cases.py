"""The edge-case rays of tests/hit_ray_cases.py, made honest before a GPU sees them (CPU).

With the oracle's flat list as the truth, every class of every scene must meet both outcomes (a class
that only hits, or only misses, checks one branch), the plane class must contain rays that lie in a
rect's plane (t = NaN, Q20), the scale class hits on both sides of t-max, and the oracle's own f64 tree
— the truth of the production band tests, which has never seen such rays either — must return the flat
list's answer for every one of them.
"""
import numpy as np
import pytest

import hit_ray_cases as hc


def _has(name, make, classes, what):
    sc, _ = hc.scene_rays(name, make, classes)
    P = hc.Prims(sc)
    return len(getattr(P, what)) > 0


@pytest.mark.parametrize("name", list(hc.CASES))
def test_every_class_meets_hits_and_misses(oracle_mod, name):
    make, classes, _ = hc.CASES[name]
    _, rays = hc.scene_rays(name, make, classes)
    flat = hc.oracle_flat(oracle_mod, name, make, classes)
    spheres = _has(name, make, classes, "r")
    assert set(rays) == set(classes)
    for cls, (r, tags) in rays.items():
        t, m = flat[cls]
        assert r.shape == (len(tags), 7) and r.dtype == np.float64
        assert len(r) >= (12 if cls == "nonfinite" else hc.N)
        share = float((m >= 0).mean())
        print("%-14s %-9s %4d rays, %5.1f %% hit, %d NaN t" % (name, cls, len(r), 100 * share, int(np.isnan(t).sum())))
        if cls in hc.HIT_SHARE and (spheres or cls == "nonfinite"):
            assert share >= hc.HIT_SHARE[cls], (name, cls, share)     # hits by construction
        else:
            assert 0.10 <= share <= 0.90, (name, cls, share)
    if "nonfinite" in rays:
        assert not np.isfinite(rays["nonfinite"][0][:, :6]).all(axis=1).any()
    for cls in set(rays) - {"nonfinite"}:
        assert np.isfinite(rays[cls][0]).all(), cls


@pytest.mark.parametrize("name", list(hc.CASES))
def test_the_edges_are_met(oracle_mod, name):
    """What each class is for is in it: zero components of both signs, origins on the planes, NaN t,
    t next to t-min and on both sides of t-max, the shutter's ends, origins outside the root box."""
    make, classes, _ = hc.CASES[name]
    sc, rays = hc.scene_rays(name, make, classes)
    flat = hc.oracle_flat(oracle_mod, name, make, classes)
    P = hc.Prims(sc)
    d = rays["axis"][0][:, 3:6]
    nz = (d == 0).sum(axis=1)
    neg = (np.signbit(d) & (d == 0)).any(axis=1)
    for zeros in (1, 2):
        assert ((nz == zeros) & neg).sum() >= 32 and ((nz == zeros) & ~neg).sum() >= 32
    o = rays["axis"][0][:, 0:3]
    outside = ((o < P.root_lo) | (o > P.root_hi)).any(axis=1)
    assert outside.sum() >= 64 and (~outside).sum() >= 64
    assert ((rays["plane"][0][:, 3:6] == 0).sum(axis=1) >= 1).all()
    if P.rects:
        t, m = flat["plane"]
        assert int((np.isnan(t) & (m >= 0)).sum()) >= 8                # rays in a rect's plane: hits with t = NaN
    # scale: the same first hit at t just below t-max (a hit) and just above it (none at that distance)
    r, tags = rays["scale"]
    t, m = flat["scale"]
    below = np.array([g == "tmax_below" for g in tags])
    above = np.array([g == "tmax_above" for g in tags])
    near = (m >= 0) & (t > hc.TMAX * (1 - 2.0 ** -9)) & (t <= hc.TMAX)
    print("%s: t-max straddle: %d of %d below hit within 2^-9 of t-max, %d of %d above miss" % (
        name, int((below & near).sum()), int(below.sum()), int((above & (m < 0)).sum()), int(above.sum())))
    assert (below & near).sum() >= 16 and (above & (m < 0)).sum() >= 16
    assert np.abs(np.log2(np.linalg.norm(r[:, 3:6], axis=1))).max() >= 39
    if "surface" in rays and len(P.small):
        t, m = flat["surface"]
        tmin = np.array([g == "tmin" for g in rays["surface"][1]])
        assert tmin.sum() >= 16                       # aimed at t = 0.001 (1 +- a few ulps): whichever side, a hit follows
    if "time" in rays:
        tm = rays["time"][0][:, 6]
        lo, hi = P.times()
        assert ((tm >= lo) & (tm <= hi)).all()
        assert (np.signbit(tm) & (tm == 0)).sum() >= 32 and (~np.signbit(tm) & (tm == 0)).sum() >= 32
        own = P.moving & (P.t0 != P.t1) & ((np.minimum(P.t0, P.t1) > lo) | (np.maximum(P.t0, P.t1) < hi))
        if own.any():                                 # a sphere whose own shutter is shorter than the camera's
            assert sum(g == "extrapolated" for g in rays["time"][1]) >= 8
    if "far" in rays:
        dist = np.linalg.norm(rays["far"][0][:, 0:3], axis=1) / P.radius
        assert (dist > 0.9e9).sum() >= 64 and ((dist > 0.9e6) & (dist < 1.1e6)).sum() >= 64
    else:
        for cls, (r, _) in rays.items():             # sphere scenes: inside the radius the box margin is sized for
            if cls != "nonfinite":
                assert np.linalg.norm(r[:, 0:3], axis=1).max() <= 4 * P.radius, cls


def test_in_plane_ray_by_the_list(oracle_mod):
    """hit_ray_cases.IN_PLANE_RAY: the list's answer is the ceiling it lies in, with t = NaN — through the
    flat list and through the oracle's tree alike — and the ray is one in_rect_plane marks."""
    ray = np.array([hc.IN_PLANE_RAY[0]])
    for make in (hc.room_static_scene, hc.room_mix_scene, hc.room_wrapped_scene):
        sc = make(hc.NX, hc.NY)
        assert hc.in_rect_plane(hc.Prims(sc), ray).all()
        o = oracle_mod.build_scene(sc)
        for flat in (True, False):
            o.set_bvh_flat(flat)
            t, m = hc.oracle_hits(o, ray)
            assert np.isnan(t[0]) and m[0] == 2                       # the third material emitted: the ceiling's


@pytest.mark.parametrize("name", list(hc.ORACLE_TREE_CASES))
def test_oracle_tree_equals_flat_list_on_edge_rays(oracle_mod, name):
    """The oracle's conservative f64 tree (oracle/rt_oracle.c, bvh_hit) against the flat list it restates:
    the same t (bit for bit, NaN = NaN) and material on every ray of every class."""
    make, classes = hc.ORACLE_TREE_CASES[name]
    sc, rays = hc.scene_rays(name, make, classes)
    flat = hc.oracle_flat(oracle_mod, name, make, classes)
    o = oracle_mod.build_scene(sc)
    o.set_bvh_flat(False)
    for cls, (r, tags) in rays.items():
        t, m = hc.oracle_hits(o, r)
        ft, fm = flat[cls]
        bad = np.flatnonzero(~hc.same_t(t, ft) | (m != fm))
        print("%-13s %-9s %4d rays, %4d hits, %d differ" % (name, cls, len(r), int((fm >= 0).sum()), len(bad)))
        assert len(bad) == 0, [(cls, tags[k], r[k].tolist(), (t[k], m[k]), (ft[k], fm[k])) for k in bad[:3]]
