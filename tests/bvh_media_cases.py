"""Scenes and rays for media forests (RT_HAS_MEDIA_BVH; no GPU): scenes with constant media
whose segments get trees of their own, their thin twins, and the edge-case rays of tests/hit_ray_cases.py and
tests/bvh_generic_cases.py built from each scene's own primitives (the media taken out: a medium is no
primitive a ray is aimed at, and its boundary is no leaf).

A thin twin is the same scene with every density 1e-300: a medium then draws its random number wherever the
full one does (the draw depends on the boundary and the closest hit so far), but -(1/density) log(xi) exceeds
any finite span, so it never reports a hit — what the oracle's probe, which has no stream, computes."""
import numpy as np

import bvh_generic_cases as bc
import hit_ray_cases as hc
from rtamd import scene as g
from rtamd import scenes
from rtamd import vec as v
from rtamd.rng import HostStream

NX, NY = 64, 36
SEED = 0x5EED0501
THIN = 1e-300
CLASSES = bc.CLASSES


def next_week_small_media(nx, ny, thin=False):
    """scenes.next_week with its two media at 6 x 6 boxes and a cluster of 60: segments of 216 box faces and
    the five leaves after them, none, and 60 instanced spheres and two more leaves."""
    return scenes.next_week(nx, ny, earth=False, media=True, boxes_per_side=6, cluster=60,
                            media_density=(THIN, THIN) if thin else (0.2, 0.0001))


def media_mix(nx, ny, thin=False):
    """Three media, four segments.  0: a 3 x 3 box field and 6 spheres under one chain (a tree).  1: 5 rects
    (below the threshold: groups beside trees).  2: 50 instanced spheres, a world-level moving sphere with
    shutter [0, 1] (a time-0 twin on a tree that is not the first) and the top face of segment 0's middle box
    listed again under the same chain (an exact tie across two trees).  3: nothing.  The media: a box under
    translate o rotate-y, a sphere, and a sphere that encloses the camera and everything else."""
    rr = HostStream(0x5EED0502)
    m = bc._three_mats()
    off = v.vec3(1, 0, 0.5)
    seg0, again = [], None
    for i in range(3):
        for j in range(3):
            p0, p1 = v.vec3(-1.5 + i, 0, -1.5 + j), v.vec3(-0.5 + i, 0.3 + rr(), -0.5 + j)
            seg0.append(g.translate(g.make_box(p0, p1, bc._lam(0.2 + 0.6 * rr(), 0.2 + 0.6 * rr(), 0.2 + 0.6 * rr())), off))
            if (i, j) == (1, 1):
                again = g.translate(g.make_xz_rect(p0[0], p1[0], p0[2], p1[2], p1[1], bc._lam(0.9, 0.1, 0.1)), off)
    for k in range(6):
        seg0.append(g.translate(g.make_sphere(v.vec3(-1 + 0.4 * k, 1.8, 0.3 * k - 0.5), 0.25, m[k % 3]), off))
    seg2 = [g.translate(g.rotate_y(g.make_sphere(v.vec3(2 * rr(), 2 * rr(), 2 * rr()), 0.1, m[k % 3]), 25), v.vec3(-3, 0.2, -2))
            for k in range(50)]
    d = (THIN, THIN, THIN) if thin else (0.8, 1.5, 0.02)
    smoke = g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(1, 1.2, 1), m[0]), -18), v.vec3(-2.5, 0, 1))
    objs = [
        g.make_bvh_node(seg0, 0, 1),
        g.make_constant_medium(smoke, d[0], g.constant_texture(v.vec3(0.9, 0.9, 0.9))),
        g.make_xz_rect(-6, 6, -6, 6, -0.01, bc._lam(0.4, 0.5, 0.3)),
        g.make_xy_rect(-4, 4, 0, 3, -4, bc._lam(0.6, 0.6, 0.3)),
        g.make_yz_rect(0, 3, -4, 4, -5, bc._lam(0.3, 0.6, 0.6)),
        g.flip_normals(g.make_yz_rect(0, 3, -4, 4, 5, bc._lam(0.6, 0.3, 0.6))),
        g.flip_normals(g.make_xz_rect(-1, 1, -1, 1, 5, g.make_diffuse_light(g.constant_texture(v.vec3(6, 6, 6))))),
        g.make_constant_medium(g.make_sphere(v.vec3(2.5, 1, -1), 0.8, m[2]), d[1], g.constant_texture(v.vec3(0.2, 0.4, 0.9))),
        g.make_bvh_node(seg2, 0, 1),
        g.make_moving_sphere(v.vec3(0, 2.6, 0), v.vec3(0.3, 3.1, -0.2), 0, 1, 0.3, m[1]),
        again,
        g.make_constant_medium(g.make_sphere(v.vec3(0, 1, 0), 100, m[2]), d[2], g.constant_texture(v.vec3(1, 1, 1))),
    ]
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


#: name -> constructor(nx, ny, thin=False)
CASES = {"next_week_small_media": next_week_small_media, "media_mix": media_mix}
#: what rt_get_tree_info reports for the forests: segments, segment_trees, sphere_leaves, generic_leaves, nodes0 > 0
EXPECTED = {"next_week_small_media": (3, 2, 4 + 2, 217 + 60), "media_mix": (4, 2, 1, 60 + 51)}


def without_media(scene):
    """The scene's primitives: its list with the media taken out."""
    return g.make_scene([o for o in scene.obj_list if o.kind != "medium"], scene.camera, scene.sky_function,
                        perlin=scene.perlin)


def tree_rotations(scene, generic_min=bc.GENERIC_MIN):
    """The forest's rotation table as rt_build.cpp fills it: per segment that has at least generic_min generic
    leaves, the rotation frames of its rects with the local axes (0 x, 1 y, 2 z) their planes are normal to."""
    table = {}
    seg = []

    def close():
        gen = [lf for lf in seg if lf.kind == "r" or lf.chain]
        if len(gen) >= generic_min:
            for lf in gen:
                if lf.kind == "r":
                    table.setdefault(bc.rotations(lf.chain), set()).add(hc.RECT_AXES[lf.data[0]][2])
        del seg[:]

    for o in scene.obj_list:
        if o.kind == "medium":
            close()
        else:
            seg.extend(bc.flatten(g.make_scene([o], scene.camera, scene.sky_function)))
    close()
    assert len(table) <= bc.MAX_ROT
    return table


def order_dependent(scene, rays):
    """rt_kernels.hip's order_dependent restated: a component that is not finite and below 1e150, or a
    direction exactly +-0 along some tree rect's normal in that rect's rotation frame."""
    r = np.asarray(rays, dtype=float)
    with np.errstate(all="ignore"):
        flag = ~(np.abs(r[:, :6]) < 1e150).all(axis=1)
        for rot, axes in tree_rotations(scene).items():
            x, y, z = r[:, 3].copy(), r[:, 4], r[:, 5].copy()
            for sn, cs in rot:                               # chain_ray's rotation of the direction
                x, z = cs * x - sn * z, sn * x + cs * z
            for ax, comp in ((0, x), (1, y), (2, z)):
                if ax in axes:
                    flag |= comp == 0.0
    return flag


_cache = {}


def scene_rays(name):
    """{class: (rays (n, 7), tags)} of a case, built from the scene's primitives; cached."""
    if name not in _cache:
        P = bc.WorldPrims(without_media(CASES[name](NX, NY)))
        out = {}
        for ci, cls in enumerate(CLASSES):
            rng = np.random.default_rng([SEED, ci])
            with np.errstate(all="ignore"):
                out[cls] = bc._BUILDERS[cls](P, rng)
        _cache[name] = out
    return _cache[name]
