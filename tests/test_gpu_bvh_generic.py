"""Rects, boxes and instanced primitives in the world tree (RT_HAS_GENERIC_BVH), on the scenes and rays of
tests/bvh_generic_cases.py.

The truth is the oracle's flat list (hit-obj-list, geometry.scm:33-50): the tree's answer must be the
list's, ties included, so t is compared bit for bit and hit / miss and material on every
ray, with no allowance.  Renders of the tree commit are compared bit for bit with renders of the groups
commit of the same scene (RTAMD_BVH_GENERIC_MIN above its leaf count, read at commit), and with the oracle
under test_gpu_parity's bounds.
"""
import numpy as np
import pytest
import torch

import bvh_generic_cases as bc
import hit_ray_cases as hc
from conftest import host_threads
from rtamd import gpu, scenes
from rtamd._lib import RtError
from test_gpu_parity import RMS_TOL, _compare

pytestmark = pytest.mark.gpu

ENV = "RTAMD_BVH_GENERIC_MIN"
SEED = 0x5EED0405
OFF = "1000000000"
RENDER_CASES = dict(bc.CASES, next_week=bc.next_week_small)


def _commit(make, monkeypatch, groups, nx=bc.NX, ny=bc.NY):
    """A fresh scene object committed with the tree (the default threshold) or with the groups."""
    if groups:
        monkeypatch.setenv(ENV, OFF)
    else:
        monkeypatch.delenv(ENV, raising=False)
    sc = make(nx, ny)
    h = gpu.upload(sc)
    monkeypatch.delenv(ENV, raising=False)
    return sc, h


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_tree_info_reports_generic_leaves(sched, monkeypatch, name):
    """The tree takes every rect and instanced sphere with a table entry; the rest stay in groups; such a
    scene walks its tree in device memory only."""
    sc, h = _commit(RENDER_CASES[name], monkeypatch, groups=False)
    ti, si = gpu.tree_info(h), gpu.scene_info(h)
    want = bc.expected_tree(sc)
    print(name, ti, "expected (spheres, generic, groups, rotations):", want)
    assert ti["generic_leaves"] > 0
    assert (ti["sphere_leaves"], ti["generic_leaves"], ti["group_leaves"], ti["rot_entries"]) == want
    assert ti["curve_leaves"] == 0 and ti["generic_min"] == bc.GENERIC_MIN
    assert 0 < ti["nodes"] <= want[0] + want[1] - 1 and 0 < ti["depth"] <= 32   # (coincident primitives share a leaf)
    assert si["leaves"] == sum(want[:3]) and si["tree_depth"] >= ti["depth"]
    assert si["extend_lds_bytes"] == 0 and si["camera_lds_bytes"] == 0 and si["bvh_solo"] == 0
    one = np.zeros((1, 7))
    one[0, 3] = 1.0
    for walk in (hc.WALK_LDS_TIME0, hc.WALK_LDS_CAMERA):
        with pytest.raises(RtError, match="LDS"):
            gpu.hit_rays(sc, one, walk=walk)
    gpu.hit_rays(sc, one, walk=hc.WALK_HBM)


def test_time0_tree_only_where_spheres_move(sched, monkeypatch):
    _, h = _commit(bc.cluster, monkeypatch, groups=False)
    ti = gpu.tree_info(h)
    assert 0 < ti["nodes0"] <= ti["sphere_leaves"] + ti["generic_leaves"] - 1 and 0 < ti["depth0"] <= 32
    _, h = _commit(bc.box_field, monkeypatch, groups=False)
    assert gpu.tree_info(h)["nodes0"] == 0


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_threshold_above_the_leaf_count_keeps_the_groups(sched, monkeypatch, name):
    sc, h = _commit(RENDER_CASES[name], monkeypatch, groups=True)
    ti = gpu.tree_info(h)
    want = bc.expected_tree(sc, generic_min=int(OFF))
    print(name, ti)
    assert ti["generic_leaves"] == 0 and ti["rot_entries"] == 0 and ti["generic_min"] == int(OFF)
    assert (ti["sphere_leaves"], ti["group_leaves"]) == (want[0], want[2])


@pytest.mark.parametrize("name", ["cornell", "cover"])
def test_existing_scenes_keep_their_commit(sched, monkeypatch, name):
    """Below the threshold nothing changes: no generic leaves, and the rt_scene_info of a commit that cannot
    take any (the threshold out of reach)."""
    infos = []
    for groups in (False, True):
        _, h = _commit(scenes.SCENES[name], monkeypatch, groups)
        ti = gpu.tree_info(h)
        assert ti["generic_leaves"] == 0 and ti["rot_entries"] == 0
        infos.append({k: x for k, x in gpu.scene_info(h).items() if not k.startswith("commit_")})
    print(name, infos[0], gpu.tree_info(h))
    assert infos[0] == infos[1]
    if name == "cornell":
        assert infos[0]["leaves"] == 18 and infos[0]["bvh_nodes"] == 0 and ti["group_leaves"] == 18
    else:
        assert infos[0]["bvh_solo"] == 1 and infos[0]["extend_lds_bytes"] > 0 and infos[0]["camera_lds_bytes"] > 0
        assert ti["group_leaves"] == 0 and ti["sphere_leaves"] == infos[0]["leaves"]


@pytest.mark.parametrize("name", list(bc.CASES))
def test_hbm_walk_equals_flat_list(sched, oracle_mod, monkeypatch, name):
    """Every ray of every class: t the same double (NaN equal to NaN), hit / miss and material equal; 0
    differences."""
    monkeypatch.delenv(ENV, raising=False)
    sc, rays = bc.scene_rays(name)
    flat = bc.oracle_flat(oracle_mod, name)
    assert gpu.tree_info(gpu.upload(sc))["generic_leaves"] > 0
    bad = []
    for c in bc.CLASSES:
        r = rays[c][0]
        et, em = flat[c]
        t, m = gpu.hit_rays(sc, r, walk=hc.WALK_HBM)
        t_bad, hit_bad, mat_bad = ~hc.same_t(t, et), (m >= 0) != (em >= 0), m != em
        print("%-9s %-9s %4d rays %4d hits %3d NaN t: t differs on %d, hit/miss on %d, material on %d" % (
            name, c, len(r), int((em >= 0).sum()), int(np.isnan(et).sum()), int(t_bad.sum()), int(hit_bad.sum()),
            int(mat_bad.sum())))
        bad += [(c, r[k].tolist(), rays[c][1][k], (et[k], int(em[k])), (t[k], int(m[k])))
                for k in np.flatnonzero(t_bad | hit_bad | mat_bad)]
    assert not bad, (len(bad), bad[:4])


def test_chain_around_a_node_flattens_to_the_same_scene(sched, monkeypatch):
    """translate o rotate-y around one make-bvh-node (the book's form) and around each of its spheres are the
    same leaves under the same chains: the same tree, and the same t and material on every ray."""
    monkeypatch.delenv(ENV, raising=False)
    sc, rays = bc.scene_rays("cluster")
    node = bc.cluster(bc.NX, bc.NY, around_node=True)
    assert gpu.tree_info(gpu.upload(node)) == gpu.tree_info(gpu.upload(sc))
    for c in bc.CLASSES:
        t0, m0 = gpu.hit_rays(sc, rays[c][0])
        t1, m1 = gpu.hit_rays(node, rays[c][0])
        assert hc.same_t(t0, t1).all() and np.array_equal(m0, m1), c


SCHEDULES = {"default": {}, "tail_only": {"tail_paths": 100000000}, "wavefront_only": {"tail_off": 1},
             "chunked_two_lanes": {"lanes": 2, "max_paths": 4096, "tail_off": 1}}


def _render(sc, nx, ny, spp):
    acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda:0")
    h = gpu.render_device(sc, nx, ny, 0, spp, SEED, acc.data_ptr())
    torch.cuda.synchronize()
    return acc.cpu().numpy(), int(gpu.stats(h).segments)


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_tree_commit_renders_what_the_groups_commit_renders(sched, monkeypatch, name):
    """48x48x8 on four schedules: bit-identical frames and equal segment counts; and the eight feature
    channels."""
    nx, ny, spp = 48, 48, 8
    tree, ht = _commit(RENDER_CASES[name], monkeypatch, groups=False, nx=nx, ny=ny)
    grp, hg = _commit(RENDER_CASES[name], monkeypatch, groups=True, nx=nx, ny=ny)
    assert gpu.tree_info(ht)["generic_leaves"] > 0 and gpu.tree_info(hg)["generic_leaves"] == 0
    for sname, opts in SCHEDULES.items():
        sched.reset_options()
        for k, x in opts.items():
            sched.set_option(k, x)
        a, sa = _render(tree, nx, ny, spp)
        b, sb = _render(grp, nx, ny, spp)
        print("%-9s %-18s segments %d / %d, pixels differing %d" % (
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


@pytest.mark.parametrize("name", ["box_field", "cluster", "city", "next_week"])
def test_tree_render_vs_oracle(sched, oracle_mod, monkeypatch, name):
    """32x32x4 against the oracle's render, under test_gpu_parity's bounds; the segment count is the oracle's
    when no pixel differs."""
    nx, ny, spp = 32, 32, 4
    sc, h = _commit(RENDER_CASES[name], monkeypatch, groups=False, nx=nx, ny=ny)
    assert gpu.tree_info(h)["generic_leaves"] > 0
    acc, segs = _render(sc, nx, ny, spp)
    ref, osegs = oracle_mod.build_scene(sc).render(nx, ny, 0, spp, SEED, nthreads=host_threads())
    rms, dmax, nbad, npx = _compare(acc, ref, spp)
    print("%s: rms=%.3e max=%.3e pixels>1e-9: %d/%d, segments %d / %d" % (name, rms, dmax, nbad, npx, segs, osegs))
    assert np.isfinite(acc).all()
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 200)
    if not (acc != ref).any():
        assert segs == osegs
