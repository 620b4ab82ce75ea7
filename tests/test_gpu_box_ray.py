"""The LDS walks' f32 box ray (scheme-raytrace_amd/csrc/rt_boxray.h: 1/d from the f32-rounded direction,
o/d one f32 product) on the rays that strain it, through the closest-hit probe (rt_hit_rays_walk, as
tests/test_gpu_hit_walks.py drives it): the time-0 tree with sign-selected planes (k_extend_lds's query) and
the all-times tree (k_camera's), SOLO and not.  Each ray's t and material must equal the oracle's flat list
walk exactly: a box culled that the ray hits shows as a miss or a farther hit.

Scenes: cover (SOLO: leafless time-0 tree), cover with its moving spheres frozen (k_camera on the time-0
tree), room_mix (leaf records, other groups beside the tree) over both LDS walks and the HBM trees; and
test_scene, whose five spheres take no tree at all (no LDS walk: it refuses them), over the walk it has.

Ray families (tests/csrc/box_ray_check.cpp has the same on single boxes, against exact arithmetic):
  tiny       one or two direction components +-0, f64 / f32 subnormal, 2^-126, 1e-30; the origin inside the
             target sphere's slab on those axes, on one of its planes, or outside it
  huge       a direction component of 1e30, or the whole direction scaled so that its largest is 1e30 (every
             t is far below t-min, so the list reports a miss: the walks must end and say the same)
  plane      origins on one to three planes of a sphere's box (c +- r), heading in, out and along
  radius     origins at |o| = R, the radius the box margin is sized for (4 x the farthest primitive + 1)
  graze      rays through a corner of a sphere's box or a point of one of its edges
"""
import numpy as np
import pytest

import hit_ray_cases as hc
from rtamd import gpu, scenes
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

SCENES = {"cover": scenes.random_scene, "cover_static": hc.static_cover_scene, "room_mix": hc.room_mix_scene,
          "test_scene": scenes.test_scene}
LDS_SCENES = ("cover", "cover_static", "room_mix")
TINY = (0.0, 5e-324, 1e-310, 1e-40, 2.0 ** -126, 1e-30)
PER_FAMILY = 205                                  # x 5 families x 4 scenes = 4100 rays
_runs = {}


def _sign(rng):
    return -1.0 if rng.integers(2) else 1.0


def _rays(P, rng):
    R = 4.0 * float(np.max(np.linalg.norm(P.c0, axis=1) + P.r)) + 1.0       # scene_radius (rt_build.cpp), spheres
    rows, fam = [], []

    def add(o, d, f):
        rows.append(np.concatenate([o, d, [0.0]]))
        fam.append(f)

    def origin_near(p):
        return p - hc.unit(rng.normal(size=3)) * rng.uniform(0.5, 6.0)

    for k in range(PER_FAMILY):
        # tiny
        i, c, r = P.pick_sphere(rng, small=(k % 8) != 7)
        p = c + 0.6 * r * hc.unit(rng.normal(size=3)) * rng.uniform()
        o = origin_near(p)
        d = (p - o) * 2.0 ** int(rng.integers(-3, 4))
        for ax in rng.permutation(3)[:1 + k % 2]:
            d[ax] = _sign(rng) * TINY[int(rng.integers(len(TINY)))]
            o[ax] = (p[ax], c[ax] - r, c[ax] + r, o[ax])[(k // 2) % 4]
        add(o, d, "tiny")
        # huge
        _, c, r = P.pick_sphere(rng)
        p = c + 0.6 * r * hc.unit(rng.normal(size=3)) * rng.uniform()
        o = origin_near(p)
        d = p - o
        ax = int(np.argmax(np.abs(d)))
        if k % 2 == 0:
            d = d * (1e30 / abs(d[ax]))
        else:                                        # nearly along one axis: the origin straight behind p
            o = p.copy()
            o[ax] -= np.sign(d[ax]) * rng.uniform(0.5, 6.0)
            d = rng.normal(size=3) * (p - o)[ax] * 1e-3
        d[ax] = np.sign(d[ax]) * 1e30
        add(o, d, "huge")
        # plane
        _, c, r = P.pick_sphere(rng)
        o = c + rng.uniform(-1.5, 1.5, size=3) * r
        for ax in rng.permutation(3)[:1 + k % 3]:
            o[ax] = c[ax] + _sign(rng) * r
        p = c + (0.0 if (k // 3) % 2 == 0 else 3.0) * r * hc.unit(rng.normal(size=3)) + 0.5 * r * rng.normal(size=3)
        d = p - o
        if (k // 6) % 3 == 2:
            d[int(rng.integers(3))] = 0.0 * _sign(rng)
        add(o, d * rng.choice([0.25, 1.0, 8.0]), "plane")
        # radius
        u = hc.unit(rng.normal(size=3))
        if k % 4 == 3:
            u = np.eye(3)[int(rng.integers(3))] * _sign(rng)
        o = R * u
        p = hc.target(P, rng) if k % 2 == 0 else hc.interior(P, rng, 0.1)
        add(o, (p - o) * rng.choice([1.0 / R, 1.0, 2.0 ** -40]), "radius")
        # graze
        _, c, r = P.pick_sphere(rng)
        p = c + r * rng.choice([-1.0, 1.0], size=3)
        if k % 2:
            ax = int(rng.integers(3))
            p[ax] = c[ax] + rng.uniform(-1.0, 1.0) * r
        o = origin_near(p)
        add(o, (p - o) * rng.choice([0.5, 1.0, 3.0]), "graze")
    return np.array(rows), np.array(fam)


def _run(oracle_mod, name):
    if name not in _runs:
        sc = SCENES[name](hc.NX, hc.NY)
        P = hc.Prims(sc)
        with np.errstate(all="ignore"):
            rays, fam = _rays(P, np.random.default_rng([hc.SEED, 77, sorted(SCENES).index(name)]))
        o = oracle_mod.build_scene(sc)
        o.set_bvh_flat(True)
        # the all-times tree is also walked at the shutter's times (the time-0 walk takes +0.0 only)
        timed = rays.copy()
        tlo, thi = P.times()
        timed[:, 6] = np.linspace(tlo, thi, len(timed))
        _runs[name] = (sc, rays, fam, hc.oracle_hits(o, rays), timed, hc.oracle_hits(o, timed))
    return _runs[name]


def _check(name, what, fam, got, want):
    t, m = got
    et, em = want
    t_bad = ~hc.same_t(t, et)
    m_bad = m != em
    for f in ("tiny", "huge", "plane", "radius", "graze"):
        k = fam == f
        print("%-10s %-22s %-6s %4d rays %4d hits: t differs on %d, material on %d" % (
            name, what, f, int(k.sum()), int((em[k] >= 0).sum()), int(t_bad[k].sum()), int(m_bad[k].sum())))
    bad = np.flatnonzero(t_bad | m_bad)
    assert len(bad) == 0, (what, len(bad), [(fam[k], (et[k], int(em[k])), (t[k], int(m[k]))) for k in bad[:4]])


@pytest.mark.parametrize("name", list(SCENES))
def test_lds_walks_equal_the_list_on_box_ray_edge_rays(sched, oracle_mod, name):
    sc, rays, fam, want, timed, want_timed = _run(oracle_mod, name)
    info = gpu.scene_info(gpu.upload(sc))
    print(name, {k: info[k] for k in ("bvh_solo", "tree0_any_time", "extend_lds_bytes", "camera_lds_bytes")})
    hits = int((want[1] >= 0).sum())
    assert len(rays) // 4 <= hits < len(rays), hits          # the rays meet the scene, and some leave it
    _check(name, "hbm walk", fam, gpu.hit_rays(sc, rays, walk=hc.WALK_HBM), want)
    _check(name, "hbm walk, shutter", fam, gpu.hit_rays(sc, timed, walk=hc.WALK_HBM), want_timed)
    if name not in LDS_SCENES:
        assert info["extend_lds_bytes"] == 0 and info["camera_lds_bytes"] == 0
        for walk in (hc.WALK_LDS_TIME0, hc.WALK_LDS_CAMERA):
            with pytest.raises(RtError, match="LDS"):
                gpu.hit_rays(sc, rays[:4], walk=walk)
        return
    assert info["extend_lds_bytes"] > 0 and info["camera_lds_bytes"] > 0
    _check(name, "time-0 tree, signed", fam, gpu.hit_rays(sc, rays, walk=hc.WALK_LDS_TIME0), want)
    _check(name, "camera tree", fam, gpu.hit_rays(sc, rays, walk=hc.WALK_LDS_CAMERA), want)
    _check(name, "camera tree, shutter", fam, gpu.hit_rays(sc, timed, walk=hc.WALK_LDS_CAMERA), want_timed)


def test_scenes_cover_solo_and_leaf_record_walks(sched):
    info = {name: gpu.scene_info(gpu.upload(SCENES[name](hc.NX, hc.NY))) for name in LDS_SCENES}
    assert {bool(i["bvh_solo"]) for i in info.values()} == {False, True}
    assert {not i["tree0_any_time"] for i in info.values()} == {False, True}     # k_camera: all-times and time-0 tree
