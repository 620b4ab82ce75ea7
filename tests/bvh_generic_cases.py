"""Scenes and edge-case rays for the world tree's generic leaves: rects, boxes and instanced primitives
(no GPU).  The scenes are small and each camera sees most of its scene; the rays are the classes of
tests/hit_ray_cases.py built from these scenes' own primitives, instanced ones taken to world space through
their chains, plus two classes of their own:

  chained    rays built in the local frame of a rect under an instance chain — in its plane (dir exactly
             zero on its normal, the origin on the plane: t = 0/0) and along its edges — and carried to world
             space through the chain (for xz rects, whose normal the rotation keeps, the world ray is
             exactly in the plane too)
  aimed      rays from inside and around the scene at points of its rects, world-level and instanced: in
             `collide` those points are where two primitives answer the same t
"""
import math

import numpy as np

import hit_ray_cases as hc
from rtamd import scene as g
from rtamd import scenes
from rtamd import vec as v
from rtamd.rng import HostStream

N = 256
SEED = 0x5EED0401
CLASSES = ("axis", "plane", "tangent", "surface", "inside", "scale", "time", "nonfinite", "chained", "aimed")
NX, NY = 64, 36
MAX_ROT = 16                               # the rotation table's entries (include/rt.h, rt_add_bvh)
GENERIC_MIN = 48                           # the default RTAMD_BVH_GENERIC_MIN


def _lam(r, gg, b):
    return g.make_lambertian(g.constant_texture(v.vec3(r, gg, b)))


def _three_mats():
    return [_lam(0.5, 0.6, 0.7), g.make_metal(g.constant_texture(v.vec3(0.8, 0.7, 0.6)), 0.2), g.make_dielectric(1.5)]


# ------------------------------------------------------------------ scenes
def box_field(nx, ny, side=8):
    """side x side boxes of seeded random heights under make-bvh-node (6 side^2 rects), three spheres of the
    three materials, a light rect, gradient sky."""
    rr = HostStream(0x5EED0402)
    w = 8.0 / side
    boxes = []
    for i in range(side):
        for j in range(side):
            x0, z0 = -4 + i * w, -4 + j * w
            boxes.append(g.make_box(v.vec3(x0, 0, z0), v.vec3(x0 + w, 0.2 + 0.8 * rr(), z0 + w),
                                    _lam(0.2 + 0.6 * rr(), 0.2 + 0.6 * rr(), 0.2 + 0.6 * rr())))
    m = _three_mats()
    objs = [g.make_bvh_node(boxes, 0, 1),
            g.make_sphere(v.vec3(-1.5, 1.6, 0), 0.5, m[0]), g.make_sphere(v.vec3(0, 1.7, 0.5), 0.5, m[1]),
            g.make_sphere(v.vec3(1.5, 1.6, 0), 0.5, m[2]),
            g.flip_normals(g.make_xz_rect(-2, 2, -2, 2, 4, g.make_diffuse_light(g.constant_texture(v.vec3(4, 4, 4)))))]
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


def instanced(objs, chain):
    """make-bvh-node over every object of objs under the chain (ops innermost first: ('r', degrees) or ('t',
    offset)), each object wrapped on its own.  The library flattens this to the same leaves under the same
    one chain as the chain around a make-bvh-node of objs, and the reference can express it: its rotate-y
    and translate give the hit the wrapped object's own material, which a bvh node does not have
    (geometry.scm:61, :537), so the oracle answers material -1 for a chain around a node."""
    def wrap(o):
        for op in chain:
            o = g.rotate_y(o, op[1]) if op[0] == "r" else g.translate(o, op[1])
        return o
    return g.make_bvh_node([wrap(o) for o in objs], 0, 1)


def cluster_spheres(n=120):
    """n small spheres in [0, 2]^3, a third of them moving, all three materials."""
    rr = HostStream(0x5EED0403)
    m = _three_mats()
    sph = []
    for i in range(n):
        c = v.vec3(2 * rr(), 2 * rr(), 2 * rr())
        r = 0.05 + 0.1 * rr()
        if i % 3 == 1:
            sph.append(g.make_moving_sphere(c, v.sum(c, v.vec3(0.3 * rr(), 0.3 * rr(), 0)), 0, 1, r, m[i % 3 if i % 2 else 0]))
        else:
            sph.append(g.make_sphere(c, r, m[i % 3]))
    return sph


#: cluster's three chains, ops innermost first
CLUSTER_CHAINS = ([("r", 20), ("t", v.vec3(-3, 0.2, -1.5))], [("r", -35), ("t", v.vec3(0.5, 0.2, -2.5))],
                  [("t", v.vec3(0.5, 0, 0)), ("r", 50), ("t", v.vec3(-1.5, 0.3, 0.5))])


def cluster(nx, ny, n=120, around_node=False):
    """One set of n spheres listed under two translate o rotate-y chains and under a three-op chain, over a
    ground rect.  around_node: each chain around one make-bvh-node of the spheres (the same flattened scene
    for the library; see `instanced` for why the oracle takes the other form)."""
    sph = cluster_spheres(n)
    objs = [g.make_xz_rect(-6, 6, -6, 6, 0, _lam(0.4, 0.5, 0.3))]
    for chain in CLUSTER_CHAINS:
        if around_node:
            o = g.make_bvh_node(sph, 0, 1)
            for op in chain:
                o = g.rotate_y(o, op[1]) if op[0] == "r" else g.translate(o, op[1])
            objs.append(o)
        else:
            objs.append(instanced(sph, chain))
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


def city(nx, ny, n_angles=12, n_boxes=40):
    """n_boxes boxes, each under its own translate o rotate-y, with n_angles distinct angles; a ground rect (the
    boxes stand on its plane) and two spheres."""
    rr = HostStream(0x5EED0404)
    objs = [g.make_xz_rect(-6, 6, -6, 6, 0, _lam(0.5, 0.5, 0.5))]
    for i in range(n_boxes):
        ang = -60.0 + 120.0 * (i % n_angles) / n_angles + 1.5
        box = g.make_box(v.vec3(0, 0, 0), v.vec3(0.4 + 0.5 * rr(), 0.3 + 1.5 * rr(), 0.4 + 0.5 * rr()),
                         _lam(0.2 + 0.7 * rr(), 0.2 + 0.7 * rr(), 0.2 + 0.7 * rr()))
        objs.append(g.translate(g.rotate_y(box, ang), v.vec3(-4.5 + 9 * rr(), 0, -4.5 + 8 * rr())))
    m = _three_mats()
    objs += [g.make_sphere(v.vec3(0, 2.4, 0), 0.5, m[2]), g.make_sphere(v.vec3(1.5, 2.2, 1), 0.4, m[1])]
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


def city40(nx, ny):
    """city with 40 distinct angles: past the rotation table's size."""
    return city(nx, ny, n_angles=40)


def collide(nx, ny):
    """Primitives that answer the same t: a rect listed twice with different materials, two boxes sharing a face
    plane with overlapping faces, a sphere listed twice (at world level, and under a chain), a sphere tangent
    to a rect at a point rays are aimed at (TANGENT_POINT), a box under a chain placed exactly on a world-level
    rect's plane; and a few more instanced boxes."""
    c = [_lam(0.1 + 0.04 * i, 0.9 - 0.04 * i, 0.5) for i in range(16)]
    objs = [
        g.make_xz_rect(-5, 5, -5, 5, 0, c[0]),                                  # the ground
        g.make_xy_rect(-2, 0, 0.5, 2, -1, c[1]), g.make_xy_rect(-2, 0, 0.5, 2, -1, c[2]),   # listed twice
        g.make_box(v.vec3(0.5, 0, -1), v.vec3(1.5, 1, 0), c[3]),               # these two share the plane x = 1.5
        g.make_box(v.vec3(1.5, 0, -1.5), v.vec3(2.5, 0.6, -0.5), c[4]),
        g.make_sphere(v.vec3(-2, 0.8, 1), 0.5, c[5]), g.make_sphere(v.vec3(-2, 0.8, 1), 0.5, c[6]),
        g.translate(g.make_sphere(v.vec3(0, 0, 0), 0.4, c[7]), v.vec3(2.5, 1.5, 1)),
        g.translate(g.make_sphere(v.vec3(0, 0, 0), 0.4, c[8]), v.vec3(2.5, 1.5, 1)),
        g.make_sphere(v.vec3(0, 0.5, 1.5), 0.5, c[9]),                          # tangent to the ground at (0, 0, 1.5)
        g.make_xy_rect(-4, 4, 0, 3, -3, c[10]),                                 # a back wall, and a box standing in its plane
        g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(1, 1.5, 0.5), c[11]), 0), v.vec3(-3.5, 0, -3)),
        g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(0.8, 0.8, 0.8), c[12]), 30), v.vec3(-0.5, 0, 0.2)),
        g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(0.6, 1.2, 0.6), c[13]), -20), v.vec3(2.5, 0, -2.5)),
        g.rotate_y(g.translate(g.make_box(v.vec3(0, 0, 0), v.vec3(0.5, 0.5, 0.5), c[14]), v.vec3(3, 0, 0)), 75),
        g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(0.7, 0.4, 0.7), c[15]), 30), v.vec3(-3, 0, 2.5)),
        g.translate(g.make_box(v.vec3(0, 0, 0), v.vec3(0.5, 0.9, 0.5), c[15]), v.vec3(3.5, 0, 2)),
    ]
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


TANGENT_POINT = (0.0, 0.0, 1.5)


def next_week_small(nx, ny):
    """scenes.next_week with the checker globe (the oracle restates no image textures)."""
    return scenes.next_week(nx, ny, earth=False)


#: name -> scene constructor (the probe scenes; renders also take next_week_small)
CASES = {"box_field": box_field, "cluster": cluster, "city": city, "city40": city40, "collide": collide}


# ------------------------------------------------------- flattened leaves
class Leaf:
    """One flattened leaf: kind 's' (c0, c1, t0, t1, r, moving) or 'r' (axis, a0, a1, b0, b1, k), its chain
    (ops outermost first: ('t', offset) / ('r', sin, cos)) and its position in the list."""

    def __init__(self, kind, data, chain, pos):
        self.kind, self.data, self.chain, self.pos = kind, data, tuple(chain), pos


def flatten(scene):
    """The scene's leaves in hit-obj-list order, as the library flattens them (rt_build.cpp, Flattener)."""
    out = []

    def walk(o, chain):
        a = o.args
        if o.kind == "sphere":
            out.append(Leaf("s", (np.array(a[0], float), np.array(a[0], float), 0.0, 1.0, abs(a[1]), False), chain, len(out)))
        elif o.kind == "moving_sphere":
            out.append(Leaf("s", (np.array(a[0], float), np.array(a[1], float), a[2], a[3], abs(a[4]), True), chain, len(out)))
        elif o.kind == "rect":
            out.append(Leaf("r", tuple(a[:6]), chain, len(out)))
        elif o.kind == "box":                        # six rects (geometry.scm:444-463)
            p0, p1 = a[0], a[1]
            for ax, (ia, ib, ik) in hc.RECT_AXES.items():
                for k in (p1[ik], p0[ik]):
                    out.append(Leaf("r", (ax, p0[ia], p1[ia], p0[ib], p1[ib], k), chain, len(out)))
        elif o.kind == "flip":
            walk(a[0], chain)
        elif o.kind == "bvh":
            for c in a[0]:
                walk(c, chain)
        elif o.kind == "translate":
            walk(a[0], chain + [("t", np.array(a[1], float))])
        elif o.kind == "rotate_y":
            rad = g.deg_to_rad(a[1])
            walk(a[0], chain + [("r", math.sin(rad), math.cos(rad))])
        else:
            raise ValueError(o.kind)

    for o in scene.obj_list:
        walk(o, [])
    return out


def to_world(chain, p, direction=False):
    """A local point (or direction) out of the chain, innermost op first (chain_hit, rt_kernels.hip)."""
    p = np.array(p, float)
    for op in reversed(chain):
        if op[0] == "t":
            if not direction:
                p = p + op[1]
        else:
            sn, cs = op[1], op[2]
            p = np.array([cs * p[0] + sn * p[2], p[1], (-sn) * p[0] + cs * p[2]])
    return p


def rotations(chain):
    return tuple((op[1], op[2]) for op in chain if op[0] == "r")


def expected_tree(scene, generic_min=GENERIC_MIN, bvh_min=16):
    """What rt_get_tree_info must report for a scene of spheres, moving spheres and rects with finite boxes:
    (sphere_leaves, generic_leaves, group_leaves, rot_entries)."""
    L = flatten(scene)
    table, gen, world_s = [], 0, 0
    for lf in L:
        if lf.kind == "s":
            if lf.chain:
                gen += 1
            else:
                world_s += 1
            continue
        rot = rotations(lf.chain)
        if rot not in table:
            if len(table) >= MAX_ROT:
                continue
            table.append(rot)
        gen += 1
    if gen >= generic_min and gen + world_s >= bvh_min:
        return world_s, gen, len(L) - world_s - gen, len(table)
    tree_s = world_s if world_s >= bvh_min else 0
    return tree_s, 0, len(L) - tree_s, 0


class WorldPrims(hc.Prims):
    """hit_ray_cases.Prims over every leaf of the scene: spheres where their chains put them (a chain is
    affine, so a moving sphere's centre(t) goes through it as its end points do), world-level rects for the
    builders that work in world axes, and the instanced rects with their chains for the local-frame rays."""

    def __init__(self, scene):                       # (restated: Prims.__init__ leaves instances out)
        L = flatten(scene)
        sph = [lf for lf in L if lf.kind == "s"]
        self.c0 = np.array([to_world(s.chain, s.data[0]) for s in sph], dtype=float).reshape(-1, 3)
        self.c1 = np.array([to_world(s.chain, s.data[1]) for s in sph], dtype=float).reshape(-1, 3)
        self.t0 = np.array([s.data[2] for s in sph], dtype=float)
        self.t1 = np.array([s.data[3] for s in sph], dtype=float)
        self.r = np.array([s.data[4] for s in sph], dtype=float)
        self.moving = np.array([s.data[5] for s in sph], dtype=bool)
        self.rects = [lf.data for lf in L if lf.kind == "r" and not lf.chain]
        self.chained = [lf for lf in L if lf.kind == "r" and lf.chain]
        self.planes = [(hc.RECT_AXES[r[0]][2], r[5]) for r in self.rects]
        self.cps = np.zeros((0, 12))
        self.width = np.zeros(0)
        cam = np.array(scene.camera.slots(), dtype=float)
        self.shutter = (float(cam[22]), float(cam[23]))
        self.small = np.flatnonzero(self.r < 100.0)
        pts = []
        for i in self.small:
            for tm in (0.0,) + self.shutter:
                c = self.centre(i, tm)
                pts += [c - self.r[i], c + self.r[i]]
        for (ax, a0, a1, b0, b1, k) in self.rects:
            pts += [hc.rect_point(ax, a0, b0, k), hc.rect_point(ax, a1, b1, k)]
        for lf in self.chained:
            ax, a0, a1, b0, b1, k = lf.data
            pts += [to_world(lf.chain, hc.rect_point(ax, a, b, k)) for a in (a0, a1) for b in (b0, b1)]
        pts = np.array(pts)
        self.lo, self.hi = pts.min(axis=0), pts.max(axis=0)
        self.root_lo, self.root_hi = self.lo.copy(), self.hi.copy()
        self.radius = float(np.linalg.norm(np.maximum(np.abs(self.lo), np.abs(self.hi))))


# ----------------------------------------------------------------- classes
def rays_chained(P, rng, n=N):
    """Local-frame in-plane and edge rays of instanced rects, carried to world space; for scenes without
    instanced rects, the same on world-level rects (an empty chain)."""
    R = hc.Rays()
    pool = P.chained or [Leaf("r", r, (), 0) for r in P.rects]
    ext = float(np.linalg.norm(P.hi - P.lo))
    for k in range(n):
        lf = pool[int(rng.integers(len(pool)))]
        ax, a0, a1, b0, b1, kk = lf.data
        ia, ib, ik = hc.RECT_AXES[ax]
        zero = 0.0 if (k % 4) < 2 else -0.0
        d = rng.normal(size=3) * rng.choice([0.3, 1.0, 3.0])
        p = hc.rect_point(ax, rng.uniform(a0, a1), rng.uniform(b0, b1), kk)
        mode = (k // 4) % 4
        if mode < 2:                                 # in the rect's plane: t = 0/0 in the local frame
            d[ik] = zero
            o = p - d * rng.uniform(0.05, 0.5) * ext / max(np.linalg.norm(d), 1e-30)
            o[ik] = kk
            if mode == 1:                            # from outside the rect's extent
                o[ia] += (a1 - a0) * rng.choice([-1.5, 1.5])
            tag = "nan_plane"
        else:                                        # in the plane of one of its edges, towards the rect
            z = ia if mode == 2 else ib
            d[z] = zero
            o = p - d * rng.uniform(0.05, 0.5) * ext / max(np.linalg.norm(d), 1e-30)
            o[z] = ((a0, a1) if z == ia else (b0, b1))[int(rng.integers(2))]
            tag = "edge"
        R.add(to_world(lf.chain, o), to_world(lf.chain, d, direction=True), 0.0, tag)
    return R.done()


def rays_aimed(P, rng, n=N):
    """At points of the scene's rects (instanced ones through their chains) and at TANGENT_POINT-like sphere
    feet, from origins inside and around the scene."""
    R = hc.Rays()
    pool = [Leaf("r", r, (), 0) for r in P.rects] + P.chained
    for k in range(n):
        if k % 8 == 7 and len(P.small):              # the lowest point of a sphere (a tangent floor's touch point)
            _, c, r = P.pick_sphere(rng)
            p = c - np.array([0.0, r, 0.0])
        else:
            lf = pool[int(rng.integers(len(pool)))]
            ax, a0, a1, b0, b1, kk = lf.data
            # interior points, and points on the rect's own edges and corners
            fa, fb = ((rng.uniform(), rng.uniform()), (rng.integers(2), rng.uniform()),
                      (rng.integers(2), rng.integers(2)))[(k // 8) % 3]
            p = to_world(lf.chain, hc.rect_point(ax, a0 + fa * (a1 - a0), b0 + fb * (b1 - b0), kk))
        o = hc.interior(P, rng, 0.3)
        if k % 2:                                    # from below / behind as often as from above
            o[1] = -abs(o[1]) - 0.1
        d = (p - o) * rng.choice([0.25, 1.0, 1.0, 4.0])
        R.add(o, d, 0.0, "aimed")
    return R.done()


_BUILDERS = dict(hc._BUILDERS, chained=rays_chained, aimed=rays_aimed)
_cache, _flat = {}, {}


def scene_rays(name):
    """(scene, {class: (rays (n, 7), tags)}) of a case: one seeded generator per (scene, class), cached."""
    if name not in _cache:
        sc = CASES[name](NX, NY)
        P = WorldPrims(sc)
        out = {}
        for ci, cls in enumerate(CLASSES):
            rng = np.random.default_rng([SEED, ci])
            with np.errstate(all="ignore"):
                out[cls] = _BUILDERS[cls](P, rng)
        _cache[name] = (sc, out)
    return _cache[name]


def oracle_flat(oracle_mod, name):
    """The flat-list truth of a case, computed once: {class: (t, mat)}."""
    if name not in _flat:
        sc, rays = scene_rays(name)
        o = oracle_mod.build_scene(sc)
        o.set_bvh_flat(True)
        _flat[name] = {c: hc.oracle_hits(o, r) for c, (r, _) in rays.items()}
    return _flat[name]
