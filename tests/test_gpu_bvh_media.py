"""Media forests (RT_HAS_MEDIA_BVH): scenes with constant media whose segments get trees of
their own, on the scenes and rays of tests/bvh_media_cases.py.

The tree commit is compared with the groups commit of the same scene (RTAMD_BVH_GENERIC_MIN above its leaf
count, read at commit): frames, feature channels and adaptive renders bit for bit, and through
rt_hit_rays_stream t, material and the number of random numbers drawn on every ray whose closest hit the
list's order cannot decide (bvh_media_cases.order_dependent).  The order-dependent rays, which the forest
scans as the list is written, media included, are pinned on the thin twins against the oracle's flat list;
renders are compared with the oracle under test_gpu_parity's bounds.
"""
import numpy as np
import pytest

import bvh_generic_cases as bc
import bvh_media_cases as mc
import hit_ray_cases as hc
from conftest import host_threads
from rtamd import gpu
from rtamd._lib import RtError
from test_gpu_bvh_generic import SCHEDULES, SEED, _commit, _render
from test_gpu_parity import RMS_TOL, _compare

pytestmark = pytest.mark.gpu

STREAM_SEED = 0x5EED0504
NAMES = list(mc.CASES)


def _thin(name):
    return lambda nx, ny: mc.CASES[name](nx, ny, thin=True)


@pytest.mark.parametrize("name", NAMES)
def test_tree_info_reports_the_forest(sched, monkeypatch, name):
    sc, h = _commit(mc.CASES[name], monkeypatch, groups=False)
    ti, si = gpu.tree_info(h), gpu.scene_info(h)
    segs, trees, spheres, generic = mc.EXPECTED[name]
    print(name, ti)
    assert ti["generic_leaves"] > 0
    assert (ti["segments"], ti["segment_trees"], ti["sphere_leaves"], ti["generic_leaves"]) == (segs, trees, spheres, generic)
    assert ti["curve_leaves"] == 0 and ti["generic_min"] == bc.GENERIC_MIN and ti["rot_entries"] == 1
    assert ti["group_leaves"] == si["leaves"] - spheres - generic
    assert 0 < ti["nodes"] <= spheres + generic - trees and 0 < ti["depth"] <= 32
    assert ti["nodes0"] > 0 and 0 < ti["depth0"] <= 32                 # both scenes hold a world-level moving sphere
    assert si["extend_lds_bytes"] == 0 and si["camera_lds_bytes"] == 0 and si["bvh_solo"] == 0
    one = np.zeros((1, 7))
    one[0, 3] = 1.0
    with pytest.raises(RtError, match="constant media"):
        gpu.hit_rays(sc, one)
    t, m, draws = gpu.hit_rays_stream(sc, one, STREAM_SEED)
    assert t.shape == m.shape == draws.shape == (1,)
    _, h = _commit(mc.CASES[name], monkeypatch, groups=True)
    ti = gpu.tree_info(h)
    assert (ti["segments"], ti["segment_trees"], ti["generic_leaves"], ti["rot_entries"], ti["nodes0"]) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("name", NAMES)
def test_tree_commit_renders_what_the_groups_commit_renders(sched, monkeypatch, name):
    """48x48x8 on four schedules: bit-identical frames and equal segment counts; the eight feature channels at
    4 passes; an adaptive render's sums and counts."""
    nx, ny, spp = 48, 48, 8
    tree, ht = _commit(mc.CASES[name], monkeypatch, groups=False, nx=nx, ny=ny)
    grp, hg = _commit(mc.CASES[name], monkeypatch, groups=True, nx=nx, ny=ny)
    assert gpu.tree_info(ht)["segment_trees"] == 2 and gpu.tree_info(hg)["segment_trees"] == 0
    for sname, opts in SCHEDULES.items():
        sched.reset_options()
        for k, x in opts.items():
            sched.set_option(k, x)
        a, sa = _render(tree, nx, ny, spp)
        b, sb = _render(grp, nx, ny, spp)
        print("%-22s %-18s segments %d / %d, pixels differing %d" % (
            name, sname, sa, sb, int((a.reshape(-1, 3) != b.reshape(-1, 3)).any(axis=1).sum())))
        assert np.isfinite(a).all() and a.sum() > 0
        assert np.array_equal(a, b), sname
        assert sa == sb, sname
    sched.reset_options()
    fa = np.zeros(nx * ny * 8)
    fb = np.zeros(nx * ny * 8)
    gpu.render_features_host(tree, nx, ny, 0, 4, SEED, fa)
    gpu.render_features_host(grp, nx, ny, 0, 4, SEED, fb)
    assert fa.reshape(-1, 8)[:, 7].sum() > 0
    assert np.array_equal(fa, fb)
    p = gpu.adaptive_params(0.05, min_spp=4, max_spp=16, batch_spp=4)
    a1, a2, ac, ar = gpu.render_adaptive_host(tree, nx, ny, p, SEED)
    b1, b2, bcnt, br = gpu.render_adaptive_host(grp, nx, ny, p, SEED)
    print(name, "adaptive", {k: ar[k] for k in ("rounds", "samples")})
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2) and np.array_equal(ac, bcnt)
    assert (ar["rounds"], ar["samples"]) == (br["rounds"], br["samples"]) and ac.max() > 4


@pytest.mark.parametrize("name", NAMES)
def test_tree_render_vs_oracle(sched, oracle_mod, monkeypatch, name):
    """32x32x4 against the oracle's render, under test_gpu_parity's bounds; the segment count is the oracle's
    when no pixel differs."""
    nx, ny, spp = 32, 32, 4
    sc, h = _commit(mc.CASES[name], monkeypatch, groups=False, nx=nx, ny=ny)
    assert gpu.tree_info(h)["segment_trees"] == 2
    acc, segs = _render(sc, nx, ny, spp)
    ref, osegs = oracle_mod.build_scene(sc).render(nx, ny, 0, spp, SEED, nthreads=host_threads())
    rms, dmax, nbad, npx = _compare(acc, ref, spp)
    print("%s: rms=%.3e max=%.3e pixels>1e-9: %d/%d, segments %d / %d" % (name, rms, dmax, nbad, npx, segs, osegs))
    assert np.isfinite(acc).all()
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 200)
    if not (acc != ref).any():
        assert segs == osegs


def _probe(make, monkeypatch, groups, rays):
    sc, h = _commit(make, monkeypatch, groups=groups)
    assert (gpu.tree_info(h)["segment_trees"] > 0) != groups
    return {c: gpu.hit_rays_stream(sc, rays[c][0], STREAM_SEED) for c in mc.CLASSES}


@pytest.mark.parametrize("name", NAMES)
def test_stream_probe_tree_equals_groups(sched, monkeypatch, name):
    """Real densities, 256 rays per class, one seed: on every ray that order_dependent does not flag, the tree
    and groups commits give the same t (the same double), material and number of draws."""
    rays = mc.scene_rays(name)
    tree = _probe(mc.CASES[name], monkeypatch, False, rays)
    grp = _probe(mc.CASES[name], monkeypatch, True, rays)
    sc = mc.CASES[name](mc.NX, mc.NY)
    bad, flagged, total, draws = [], 0, 0, 0
    for c in mc.CLASSES:
        f = mc.order_dependent(sc, rays[c][0])
        (t, m, d), (gt, gm, gd) = tree[c], grp[c]
        diff = ~f & (~hc.same_t(t, gt) | (m != gm) | (d != gd))
        print("%-22s %-9s %3d rays, %3d flagged, %3d hits, draws %4d: differ on %d" % (
            name, c, len(f), int(f.sum()), int((m >= 0).sum()), int(d.sum()), int(diff.sum())))
        bad += [(c, rays[c][0][k].tolist(), (t[k], int(m[k]), int(d[k])), (gt[k], int(gm[k]), int(gd[k])))
                for k in np.flatnonzero(diff)]
        flagged += int(f.sum())
        total += len(f)
        draws += int(d[~f].sum())
    assert flagged < total / 2
    assert draws > 0
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("name", NAMES)
def test_thin_twin_equals_the_flat_list(sched, oracle_mod, monkeypatch, name):
    """Every density 1e-300: a medium draws where it would and never hits, which is the oracle's probe.  Every
    ray of every class (the order-dependent ones included; of `nonfinite` those that drew nothing: an
    infinite span lets even a thin medium hit): t the same double, hit / miss and material equal; the draws
    of the rays order_dependent does not flag equal the groups commit's."""
    rays = mc.scene_rays(name)
    tree = _probe(_thin(name), monkeypatch, False, rays)
    grp = _probe(_thin(name), monkeypatch, True, rays)
    sc = _thin(name)(mc.NX, mc.NY)
    o = oracle_mod.build_scene(sc)
    o.set_bvh_flat(True)
    bad, draws = [], 0
    for c in mc.CLASSES:
        r = rays[c][0]
        et, em = hc.oracle_hits(o, r)
        t, m, d = tree[c]
        f = mc.order_dependent(sc, r)
        take = d == 0 if c == "nonfinite" else np.ones(len(r), dtype=bool)
        diff = take & (~hc.same_t(t, et) | ((m >= 0) != (em >= 0)) | (m != em))
        ddiff = ~f & (d != grp[c][2])
        print("%-22s %-9s %3d rays, %3d flagged, %3d compared, %3d NaN t, draws %4d: differ on %d, draws on %d" % (
            name, c, len(r), int(f.sum()), int(take.sum()), int(np.isnan(et).sum()), int(d.sum()), int(diff.sum()),
            int(ddiff.sum())))
        bad += [(c, r[k].tolist(), rays[c][1][k], (et[k], int(em[k])), (t[k], int(m[k]), int(d[k])))
                for k in np.flatnonzero(diff | ddiff)]
        draws += int(d.sum())
    assert draws > 0
    assert not bad, (len(bad), bad[:4])


def test_time0_twin_of_a_later_tree(sched, monkeypatch):
    """Rays through media_mix's moving sphere (in the second tree) at times +0.0, -0.0 and 0.5: only +0.0 walks
    the twin; the tree commit answers as the groups commit does."""
    rng = np.random.default_rng(0x5EED0505)
    rays = []
    for tm in (0.0, -0.0, 0.5):
        c = np.array([0, 2.6, 0]) + np.array([0.3, 0.5, -0.2]) * tm
        for _ in range(64):
            o = c + 6 * hc.unit(rng.normal(size=3))
            p = c + 0.32 * rng.uniform(-1, 1, size=3)                    # at and just around the sphere
            rays.append(np.concatenate([o, (p - o) * rng.choice([0.5, 1.0, 2.0]), [tm]]))
    rays = np.array(rays)
    assert not mc.order_dependent(mc.media_mix(mc.NX, mc.NY), rays).any()
    sc, h = _commit(mc.media_mix, monkeypatch, groups=False)
    assert gpu.tree_info(h)["nodes0"] > 0
    t, m, d = gpu.hit_rays_stream(sc, rays, STREAM_SEED)
    grp, _ = _commit(mc.media_mix, monkeypatch, groups=True)
    gt, gm, gd = gpu.hit_rays_stream(grp, rays, STREAM_SEED)
    print("hits per time:", [int((m[k * 64:(k + 1) * 64] >= 0).sum()) for k in range(3)], "draws", int(d.sum()))
    assert (m >= 0).sum() > 96
    assert hc.same_t(t, gt).all() and np.array_equal(m, gm) and np.array_equal(d, gd)
