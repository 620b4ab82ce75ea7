"""Edge-case rays for the closest-hit walks, and the scenes they are sent through (no GPU).

Camera rays and scattered rays have random directions from random interior points, so whole renders
never put a ray on a box plane, along an axis, tangent to a sphere or next to t-max.  Here every class
of ray is built from the scene's own primitives, so that the edge is actually met:

  axis       one, then two direction components exactly +0.0, and the same with -0.0; origins inside
             and outside the tree's root box
  plane      axis rays whose origin coordinate on a zero axis equals a sphere's c +- r or c, a rect's k
             (the ray lies in the rect's plane: t = 0/0 = NaN passes every comparison, Q20) or one of
             its edges a0 / a1 / b0 / b1
  tangent    rays through c + r (1 +- 2^-k) u with u perpendicular to dir, k = 20, 30, 40, 52 (for curve
             scenes: through a curve point + (width/2) (1 +- 2^-k) u)
  surface    origins on a sphere or rect (a previous hit point o + t d), outward, inward and grazing;
             and hits whose t lies within a few ulps of t-min = 0.001
  inside     origins at a sphere's centre and inside spheres (the second root)
  scale      generic rays with dir scaled by 2^+-40, and rays with |dir| = D / t-max (1 +- 2^-k) for a
             hit at distance D: t just below and just above t-max = 999999999999
  time       times +0.0, -0.0, the camera shutter's ends and middle, and times outside a sphere's own
             shutter (extrapolated centres), aimed at the spheres where they are at that time
  far        curve scenes only (the box ray that serves rays from anywhere): origins 1e6 and 1e9 scene
             radii away, aimed back at the scene, |dir| below and above 1
  nonfinite  a dozen rays with a NaN or +-inf component in dir or o (sphere / rect scenes only: there
             every loop is bounded by the tree or list size, not by ray values)

Ray times stay inside [min(t0, t1, 0), max(t0, t1, 0)] of the camera shutter: the all-times trees (the
library's, rt_build.cpp, and the oracle's, scene_prepare) bound a moving sphere over those times only,
so a ray of another time is outside what either tree is built for.  Origins of sphere scenes stay inside
the radius the f32 box margin is sized for (scene_radius, rt_build.cpp: 4 x the farthest primitive).
"""
import numpy as np

from rtamd import scene as g
from rtamd import scenes
from rtamd import vec as v
from rtamd.rng import HostStream

TMIN, TMAX = 0.001, 999999999999.0
SEED = 0x5EED0301
N = 256                                  # rays per class
WALK_HBM, WALK_LDS_TIME0, WALK_LDS_CAMERA = 0, 1, 2

CLASSES = ("axis", "plane", "tangent", "surface", "inside", "scale", "time", "far", "nonfinite")
#: rect axis -> (index of a, of b, of k) in xyz (geometry.scm:376-431)
RECT_AXES = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}


# ------------------------------------------------------------------ scenes
def moving_mix_scene(nx, ny):
    """Moving spheres whose shutters do not start at 0 (center(0) is an
    extrapolation), a degenerate shutter (t0 = t1: center(0) is NaN, never
    hit), static spheres, all three materials, and a camera shutter [0, 1]."""
    mats = _mix_mats()
    objs = [g.make_sphere(v.vec3(0, -1000, 0), 1000, mats[0])] + _mix_spheres(False, mats)
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


def _mix_mats():
    return [g.make_lambertian(g.constant_texture(v.vec3(0.5, 0.6, 0.7))),
            g.make_metal(g.constant_texture(v.vec3(0.8, 0.7, 0.6)), 0.3), g.make_dielectric(1.5)]


def _mix_spheres(static, mats=None):
    """moving_mix_scene's 60 random spheres and its degenerate one; static: each frozen where it starts."""
    rr = HostStream(0x5EED0101)
    mats = mats or _mix_mats()
    objs = []
    for i in range(60):
        c0 = v.vec3(rr() * 8 - 4, 0.2 + rr() * 0.5, rr() * 8 - 4)
        c1 = v.sum(c0, v.vec3(rr() - 0.5, rr(), rr() - 0.5))
        m = mats[i % 3]
        r, t0, t1 = ((0.25, None, None), (0.2, 0.5, 1.5), (0.3, -1.0, 0.25), (0.2, 0.0, 1.0))[i % 4]
        if t0 is None or static:
            objs.append(g.make_sphere(c0, r, m))
        else:
            objs.append(g.make_moving_sphere(c0, c1, t0, t1, r, m))
    if static:
        objs.append(g.make_sphere(v.vec3(0, 1, 0), 0.5, mats[0]))
    else:
        objs.append(g.make_moving_sphere(v.vec3(0, 1, 0), v.vec3(0, 2, 0), 0.5, 0.5, 0.5, mats[0]))
    return objs


def static_cover_scene(nx, ny):
    """The cover scene with every moving sphere frozen where it starts: no
    moving spheres, so the time-0 tree serves camera rays too (k_camera<false>)."""
    sc = scenes.random_scene(nx, ny)
    objs = [g.make_sphere(o.args[0], o.args[4], o.args[5]) if o.kind == "moving_sphere" else o
            for o in sc.obj_list]
    return g.make_scene(objs, sc.camera, sc.sky_function)


def many_spheres_scene(nx, ny):
    """2000 small spheres of all three materials: the trees outgrow the LDS
    kernels' budget, so every launch takes the HBM-tree kernels."""
    rr = HostStream(0x5EED0102)
    mats = [g.make_lambertian(g.constant_texture(v.vec3(0.6, 0.5, 0.4))),
            g.make_metal(g.constant_texture(v.vec3(0.8, 0.8, 0.7)), 0.2), g.make_dielectric(1.5)]
    objs = [g.make_sphere(v.vec3(0, -1000, 0), 1000, mats[0])]
    for i in range(2000):
        objs.append(g.make_sphere(v.vec3(rr() * 20 - 10, rr() * 2, rr() * 20 - 10), 0.05 + 0.1 * rr(), mats[i % 3]))
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


def room_mix_scene(nx, ny, static=False, wrap=False):
    """A world of several closest-hit groups: five Cornell-style rects around the spheres (one flipped, the
    front open), a rotated and translated box, and moving_mix_scene's 60 random spheres with their shutters
    (static: frozen).  Every rect has its own material, so a hit on the wrong one shows.
    wrap: the spheres under a reference-level make-bvh-node (the oracle then walks its own tree)."""
    tex = [g.constant_texture(v.vec3(0.1 + 0.1 * i, 0.5, 0.9 - 0.1 * i)) for i in range(6)]
    walls = [g.make_lambertian(t) for t in tex]
    objs = [g.flip_normals(g.make_yz_rect(-0.5, 5, -6, 6, 6, walls[0])),
            g.make_yz_rect(-0.5, 5, -6, 6, -6, walls[1]),
            g.make_xz_rect(-6, 6, -6, 6, 5, walls[2]),
            g.make_xz_rect(-6, 6, -6, 6, -0.5, walls[3]),
            g.make_xy_rect(-6, 6, -0.5, 5, 6, walls[4]),
            g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(1.5, 3, 1.5), walls[5]), 15),
                        v.vec3(2, -0.5, 2.5))]
    sph = _mix_spheres(static)
    objs += [g.make_bvh_node(sph, 0, 1)] if wrap else sph
    return g.make_scene(objs, scenes.camera_for(nx, ny), g.sky_color)


def room_static_scene(nx, ny):
    return room_mix_scene(nx, ny, static=True)


def room_wrapped_scene(nx, ny):
    return room_mix_scene(nx, ny, wrap=True)


_SPHERE_CLASSES = ("axis", "plane", "tangent", "surface", "inside", "scale", "time", "nonfinite")
_CURVE_CLASSES = ("axis", "plane", "tangent", "surface", "inside", "scale", "far")
_LDS = (WALK_HBM, WALK_LDS_TIME0, WALK_LDS_CAMERA)
#: name -> (scene constructor, ray classes, walks the scene supports)
CASES = {
    "cover": (scenes.random_scene, _SPHERE_CLASSES, _LDS),                  # k_extend_lds<1>, k_camera<1,1>
    "cover_static": (static_cover_scene, _SPHERE_CLASSES, _LDS),            # k_camera<0,1>
    "room_mix": (room_mix_scene, _SPHERE_CLASSES, _LDS),                    # k_extend_lds<0>, k_camera<1,0>
    "room_static": (room_static_scene, _SPHERE_CLASSES, _LDS),              # k_camera<0,0>
    "many_spheres": (many_spheres_scene, _SPHERE_CLASSES, (WALK_HBM,)),
    "curves_small": (scenes.cornell_curves_small, _CURVE_CLASSES, (WALK_HBM,)),
    "cornell_bezier": (scenes.cornell_bezier, _CURVE_CLASSES, (WALK_HBM,)),
}
#: scenes only the oracle's own tree is checked on (tests/test_hit_ray_cases.py)
ORACLE_TREE_CASES = {
    "bvh_sah": (scenes.test_scene_bvh_sah, _SPHERE_CLASSES),
    "curves_small": (scenes.cornell_curves_small, _CURVE_CLASSES),
    "room_wrapped": (room_wrapped_scene, _SPHERE_CLASSES),
}
#: The smallest ray found on which the library's closest hit was not the list's (room_static / room_mix): it
#: lies in the ceiling's plane (y = 5, dy = 0) and runs into the wall x = -6 at t = 6.  hit-obj-list meets the
#: wall first, then the ceiling, whose t = 0/0 = NaN passes both comparisons and becomes the closest hit; no
#: later object passes (t > NaN is false, but the floor's t is -inf and the back wall's bounds fail): (NaN,
#: ceiling).  The library groups the world's leaves by type (rt_build.cpp, emit_groups: xy, xz, then yz
#: rects), so it meets the ceiling before the wall, whose t = 6 then passes `t > NaN`: (6, wall).
IN_PLANE_RAY = ((0.0, 5.0, 0.0, -1.0, 0.0, 0.0, 0.0), "ceiling")

#: classes that hit by construction -> the least share of hits, in place of the 10 % / 10 % rule.  inside: an
#: origin strictly inside a sphere (or at its centre) has that sphere's far root ahead of it, whatever the
#: direction.  nonfinite: a dozen rays, there to terminate and agree, not to hit.
HIT_SHARE = {"inside": 1.0, "nonfinite": 0.0}
NX, NY = 64, 36


# -------------------------------------------------------------- primitives
class Prims:
    """The scene's spheres, rects and curves as arrays (instances and boxes are left out: rays are
    built from world-level primitives)."""

    def __init__(self, scene):
        sph, rects, cps, wid = [], [], [], []
        planes = []                                  # (axis, k) of every rect plane in world coordinates

        def walk(o, dy=0.0, level=True):
            a = o.args
            if o.kind == "translate":
                walk(a[0], dy + a[1][1], level)
            elif o.kind == "rotate_y":               # keeps the y planes only
                walk(a[0], dy, False)
            elif o.kind == "box":                    # six rects (geometry.scm:444-463)
                planes.extend([(1, a[0][1] + dy), (1, a[1][1] + dy)])
                if level:
                    planes.extend([(0, a[0][0]), (0, a[1][0]), (2, a[0][2]), (2, a[1][2])])
            elif o.kind == "sphere":
                sph.append((a[0], a[0], 0.0, 1.0, abs(a[1]), 0))
            elif o.kind == "moving_sphere":
                sph.append((a[0], a[1], a[2], a[3], abs(a[4]), 1))
            elif o.kind == "rect":
                rects.append(tuple(a[:6]))
                planes.append((RECT_AXES[a[0]][2], a[5]))
            elif o.kind == "flip":
                walk(a[0], dy, level)
            elif o.kind == "bvh":
                for c in a[0]:
                    walk(c)
            elif o.kind == "curves":
                cps.extend(np.asarray(a[0]).reshape(-1, 12))
                wid.extend([a[1]] * len(a[0]))
            elif o.kind == "bezier":
                cps.append(np.concatenate([np.asarray(p, dtype=float) for p in a[:4]]))
                wid.append(a[4])

        for o in scene.obj_list:
            walk(o)
        self.c0 = np.array([s[0] for s in sph], dtype=float).reshape(-1, 3)
        self.c1 = np.array([s[1] for s in sph], dtype=float).reshape(-1, 3)
        self.t0 = np.array([s[2] for s in sph], dtype=float)
        self.t1 = np.array([s[3] for s in sph], dtype=float)
        self.r = np.array([s[4] for s in sph], dtype=float)
        self.moving = np.array([s[5] for s in sph], dtype=bool)
        self.rects = rects
        self.planes = planes
        self.cps = np.array(cps, dtype=float).reshape(-1, 12)
        self.width = np.array(wid, dtype=float)
        cam = np.array(scene.camera.slots(), dtype=float)
        self.shutter = (float(cam[22]), float(cam[23]))
        # small things (not a ground sphere): where rays are aimed, and the box origins are drawn from
        pts = []
        self.small = np.flatnonzero(self.r < 100.0)
        with np.errstate(all="ignore"):
            for i in self.small:
                for tm in (0.0,) + self.shutter:
                    c = self.centre(i, tm)
                    if np.isfinite(c).all():
                        pts += [c - self.r[i], c + self.r[i]]
        for (ax, a0, a1, b0, b1, k) in rects:
            pts += [rect_point(ax, a0, b0, k), rect_point(ax, a1, b1, k)]
        if len(self.cps):
            q = self.cps.reshape(-1, 3)
            pts += [q.min(axis=0), q.max(axis=0)]
        pts = np.array(pts)
        self.lo, self.hi = pts.min(axis=0), pts.max(axis=0)
        # the tree's root box: every sphere (the ground included) or every curve
        if len(self.r):
            with np.errstate(all="ignore"):
                ok = np.isfinite(self.c0).all(axis=1)
            self.root_lo = np.minimum(self.lo, (self.c0[ok] - self.r[ok, None]).min(axis=0))
            self.root_hi = np.maximum(self.hi, (self.c0[ok] + self.r[ok, None]).max(axis=0))
        else:
            self.root_lo, self.root_hi = self.lo.copy(), self.hi.copy()
        self.radius = float(np.linalg.norm(np.maximum(np.abs(self.root_lo), np.abs(self.root_hi))))

    def centre(self, i, tm):
        """center(time) of sphere i (geometry.scm:181-184); NaN for a degenerate shutter."""
        if not self.moving[i]:
            return self.c0[i]
        with np.errstate(all="ignore"):
            return self.c0[i] + (self.c1[i] - self.c0[i]) * ((tm - self.t0[i]) / (self.t1[i] - self.t0[i]))

    def pick_sphere(self, rng, tm=0.0, small=True):
        """A sphere whose centre at time tm is finite: (index, centre, radius)."""
        pool = self.small if small and len(self.small) else np.arange(len(self.r))
        while True:
            i = int(rng.choice(pool))
            c = self.centre(i, tm)
            if np.isfinite(c).all():
                return i, c, self.r[i]

    def times(self):
        t0, t1 = self.shutter
        return min(t0, t1, 0.0), max(t0, t1, 0.0)


def in_rect_plane(P, rays):
    """Rays that lie in the plane of one of the scene's rects (a box face included): dir is exactly zero
    on the plane's axis and the origin is on it, so that rect's t is 0/0 = NaN (Q20)."""
    rays = np.asarray(rays)
    m = np.zeros(len(rays), dtype=bool)
    for ax, k in P.planes:
        m |= (rays[:, 3 + ax] == 0) & (rays[:, ax] == k)
    return m


def rect_point(axis, a, b, k):
    ia, ib, ik = RECT_AXES[axis]
    p = np.zeros(3)
    p[ia], p[ib], p[ik] = a, b, k
    return p


def bezier_point(cp, u):
    a, b, c, d = cp[0:3], cp[3:6], cp[6:9], cp[9:12]
    w = 1.0 - u
    return w * w * w * a + 3 * w * w * u * b + 3 * w * u * u * c + u * u * u * d


def unit(x):
    return x / np.linalg.norm(x)


def perp(d, rng):
    """A unit vector perpendicular to d."""
    while True:
        u = np.cross(d, rng.normal(size=3))
        n = np.linalg.norm(u)
        if n > 1e-3 * np.linalg.norm(d):
            return u / n


def target(P, rng, tm=0.0):
    """A point inside something: in a small sphere (where it is at time tm), on a rect, on a curve."""
    kinds = [k for k, n in (("s", len(P.small)), ("r", len(P.rects)), ("c", len(P.cps))) if n]
    kind = kinds[int(rng.integers(len(kinds)))]
    if kind == "s":
        _, c, r = P.pick_sphere(rng, tm)
        return c + 0.6 * r * unit(rng.normal(size=3)) * rng.uniform()
    if kind == "r":
        ax, a0, a1, b0, b1, k = P.rects[int(rng.integers(len(P.rects)))]
        return rect_point(ax, rng.uniform(a0, a1), rng.uniform(b0, b1), k)
    return bezier_point(P.cps[int(rng.integers(len(P.cps)))], rng.uniform())


def interior(P, rng, grow=0.0):
    ext = P.hi - P.lo
    return rng.uniform(P.lo - grow * ext, P.hi + grow * ext)


def escape_dir(P, rng):
    """A direction that leaves the scene without meeting much: towards the open front of a Cornell-style
    room (-z), or nearly level and slightly upward over a ground sphere."""
    if len(P.rects):
        e = 0.15 * rng.normal(size=3)
        return unit(np.array([e[0], abs(e[1]), -1.0]))
    h = rng.normal(size=3) * np.array([1.0, 0.0, 1.0])
    return unit(unit(h) + np.array([0.0, rng.uniform(0.05, 0.2), 0.0]))


def back_out(P, p, d, rng):
    """An origin on the line p - s d that lies outside the tree's root box (s > 0)."""
    s = np.inf
    for k in range(3):
        if d[k] > 0:
            s = min(s, (p[k] - P.root_lo[k]) / d[k])
        elif d[k] < 0:
            s = min(s, (p[k] - P.root_hi[k]) / d[k])
    s = max(s, 0.0) * 1.25 + 0.5 * float(np.linalg.norm(P.hi - P.lo)) / float(np.linalg.norm(d))
    return p - s * d


class Rays:
    def __init__(self):
        self.rows, self.tags = [], []

    def add(self, o, d, tm=0.0, tag=""):
        self.rows.append(np.concatenate([np.asarray(o, dtype=float), np.asarray(d, dtype=float), [tm]]))
        self.tags.append(tag)

    def done(self):
        return np.array(self.rows).reshape(-1, 7), self.tags


def _axis_dir(rng, k, zero):
    """A direction with component(s) exactly zero (signed): k % 4 -> one +0, two +0, one -0, two -0."""
    d = rng.normal(size=3) * rng.choice([0.3, 1.0, 3.0])
    axes = rng.permutation(3)[:1 + (k % 2)]
    d[axes] = zero
    return d, axes


# ----------------------------------------------------------------- classes
def rays_axis(P, rng, n=N):
    R = Rays()
    for k in range(n):
        zero = 0.0 if (k % 4) < 2 else -0.0
        d, _ = _axis_dir(rng, k, zero)
        outside = (k // 4) % 2 == 1
        if (k // 8) % 2 == 0:                       # through something
            p = target(P, rng)
            o = back_out(P, p, d, rng) if outside else p - d * rng.uniform(0.2, 2.0) * np.linalg.norm(P.hi - P.lo) / 8
        else:                                       # from anywhere
            o = interior(P, rng, 0.1)
            if outside:
                o = back_out(P, o, d if k % 16 < 12 else -d, rng)
        R.add(o, d, 0.0, "outside" if outside else "inside")
    return R.done()


def _leaving_plane_ray(P, rng, k, zero):
    """Room scenes, where nearly every ray meets a wall: an origin in front of the opening, its x on a
    sphere's plane or on a rect edge that no wall lies in, heading away with dx (and dy) exactly zero."""
    d = escape_dir(P, rng) * rng.choice([0.3, 1.0, 3.0])
    d[[0] if k % 2 == 0 else [0, 1]] = zero
    o = interior(P, rng)
    o[2] = P.lo[2] - rng.uniform(0.1, 0.5) * (P.hi[2] - P.lo[2])
    if len(P.small):
        _, c, r = P.pick_sphere(rng)
        o[0] = (c[0] - r, c[0] + r, c[0])[(k // 32) % 3]
    else:
        walls = {r[5] for r in P.rects if RECT_AXES[r[0]][2] == 0}
        edges = [e for r in P.rects for ax, e in ((RECT_AXES[r[0]][0], r[1]), (RECT_AXES[r[0]][0], r[2]),
                                                  (RECT_AXES[r[0]][1], r[3]), (RECT_AXES[r[0]][1], r[4]))
                 if ax == 0 and e not in walls]
        o[0] = edges[int(rng.integers(len(edges)))]
    return o, d


def rays_plane(P, rng, n=N):
    R = Rays()
    ext = float(np.linalg.norm(P.hi - P.lo))
    for k in range(n):
        zero = 0.0 if (k % 4) < 2 else -0.0
        if len(P.rects) and (k // 16) % 4 == 3:
            R.add(*_leaving_plane_ray(P, rng, k, zero), 0.0, "leaving")
            continue
        d, axes = _axis_dir(rng, k, zero)
        if (k // 8) % 2 == 1:                       # leaving the scene, so that some of these rays miss
            d = escape_dir(P, rng) * max(np.linalg.norm(d), 0.1)
            if len(P.rects):                        # (a room opens along z: that component stays)
                axes = rng.permutation(2)[:len(axes)]
            d[axes] = zero
        use_rect = len(P.rects) and (not len(P.small) or (k // 4) % 2 == 1)
        if use_rect:
            ax, a0, a1, b0, b1, kk = P.rects[int(rng.integers(len(P.rects)))]
            ia, ib, ik = RECT_AXES[ax]
            z = int(axes[0])
            p = rect_point(ax, rng.uniform(a0, a1), rng.uniform(b0, b1), kk)
            o = p - d * rng.uniform(0.05, 0.5) * ext / max(np.linalg.norm(d), 1e-30)
            if z == ik:                             # the ray lies in the rect's plane: t = 0/0
                o[ik] = kk
                tag = "nan_plane"
            else:                                   # the ray runs in the plane of one of the rect's edges
                edge = (a0, a1) if z == ia else (b0, b1)
                o[z] = edge[int(rng.integers(2))]
                tag = "edge"
            if (k // 8) % 4 == 3:                   # and some from outside the rect's extent
                o = o + (rng.uniform(0.3, 0.8) * ext) * np.where(np.arange(3) == z, 0.0, rng.choice([-1.0, 1.0], 3))
        else:
            i, c, r = P.pick_sphere(rng, 0.0, small=(k % 16) != 15)
            z = int(axes[0])
            o = c + rng.normal(size=3) * r * 0.7 - d * rng.uniform(0.5, 4.0) * min(r, ext) / np.linalg.norm(d)
            o[z] = (c[z] - r, c[z] + r, c[z])[(k // 8) % 3]
            tag = ("lo", "hi", "centre")[(k // 8) % 3]
            if len(axes) == 2 and (k // 8) % 2:     # two zero axes: on two box planes at once (a box edge)
                z2 = int(axes[1])
                o[z2] = c[z2] + r * rng.choice([-1.0, 1.0])
        R.add(o, d, 0.0, tag)
    return R.done()


def rays_tangent(P, rng, n=N):
    R = Rays()
    for k in range(n):
        d = rng.normal(size=3) * (1.0, 0.25, 7.0)[k % 3]
        if (k // 3) % 2 == 0:
            d = unit(d) * np.linalg.norm(d)
        # (a curve's ribbon ends where its subdivision to width / 20 puts it, not at width / 2 exactly:
        # curve scenes also pass clearly inside and outside it)
        e = ((20, 30, 40, 52) if len(P.small) else (-2, 1, 20, 52))[(k // 6) % 4]
        side = 1.0 - 2.0 ** -e if (k // 24) % 2 == 0 else 1.0 + 2.0 ** -e
        if len(P.small):
            _, c, r = P.pick_sphere(rng)
        else:
            j = int(rng.integers(len(P.cps)))
            c, r = bezier_point(P.cps[j], rng.uniform()), P.width[j] / 2
        u = perp(d, rng)
        far = rng.uniform(1.5, 6.0)
        if (k // 48) % 2 == 1 or e < 0:             # leaving the scene: past the sphere there is nothing to hit
            d = escape_dir(P, rng) * np.linalg.norm(d)
            u = perp(d, rng)
            u = u if u[1] >= 0 else -u              # (and the origin stays above the ground)
            far = rng.uniform(1.5, 3.0)
        p = c + (r * side) * u
        R.add(p - (far * r / np.linalg.norm(d)) * d, d, 0.0, "in" if side < 1 else "out")
    return R.done()


def _sphere_root(o, d, c, r):
    """The sphere's nearer root as geometry.scm:146-171 computes it, or None."""
    oc = o - c
    a, b, cc = d @ d, oc @ d, oc @ oc - r * r
    disc = b * b - a * cc
    if not disc > 0:
        return None
    return (-b - np.sqrt(disc)) / a


def rays_surface(P, rng, n=N):
    R = Rays()
    k = 0
    while len(R.rows) < n:
        k += 1
        mode = k % 8
        if len(P.small) and (mode < 6 or not len(P.rects)):
            _, c, r = P.pick_sphere(rng)
            o0 = c + unit(rng.normal(size=3)) * r * rng.uniform(2.0, 6.0)
            d0 = (c + rng.normal(size=3) * 0.5 * r) - o0
            t = _sphere_root(o0, d0, c, r)
            if t is None:
                continue
            p = o0 + t * d0                          # the hit point a scattered ray starts from
            nrm = (p - c) / r
            if mode in (4, 5):                       # a hit whose t is a few ulps either side of t-min
                dd = unit(d0)
                j = int(rng.integers(-6, 7))
                R.add(p - dd * (TMIN * (1.0 + j * 2.0 ** -52)), dd, 0.0, "tmin")
                continue
        elif len(P.rects):
            ax, a0, a1, b0, b1, kk = P.rects[int(rng.integers(len(P.rects)))]
            p = rect_point(ax, rng.uniform(a0, a1), rng.uniform(b0, b1), kk)
            nrm = np.zeros(3)
            nrm[RECT_AXES[ax][2]] = rng.choice([-1.0, 1.0])
        else:                                        # curve scenes without rects do not occur; curves: a hull point
            j = int(rng.integers(len(P.cps)))
            p = bezier_point(P.cps[j], rng.uniform())
            nrm = unit(rng.normal(size=3))
        way = k % 3
        if way == 0:
            d = nrm + 0.9 * unit(rng.normal(size=3))             # outward
        elif way == 1:
            d = -nrm + 0.9 * unit(rng.normal(size=3))            # inward
        else:
            d = perp(nrm, rng) + nrm * rng.choice([-1.0, 1.0]) * 2.0 ** -int(rng.integers(10, 50))   # grazing
        R.add(p, d * rng.choice([0.5, 1.0, 2.0]), 0.0, ("out", "in", "graze")[way])
    return R.done()


def rays_inside(P, rng, n=N):
    R = Rays()
    for k in range(n):
        if len(P.r):
            _, c, r = P.pick_sphere(rng, 0.0, small=(k % 8) != 7)
            o = c if k % 2 == 0 else c + unit(rng.normal(size=3)) * r * rng.uniform(0.0, 0.9)
            tag = "centre" if k % 2 == 0 else "inside"
        else:                                        # curves: a point of the curve itself
            j = int(rng.integers(len(P.cps)))
            o, tag = bezier_point(P.cps[j], rng.uniform()), "curve"
        d = unit(rng.normal(size=3)) if len(P.r) or k % 2 else escape_dir(P, rng)
        R.add(o, d * rng.choice([0.1, 1.0, 4.0]), 0.0, tag)     # (the far root stays beyond t-min: r >= 0.05)
    return R.done()


def rays_scale(P, rng, n=N):
    R = Rays()
    ext = float(np.linalg.norm(P.hi - P.lo))
    k = 0
    while len(R.rows) < n:
        k += 1
        if k % 2 == 0:                               # generic rays, exactly scaled
            d = rng.normal(size=3)
            p = target(P, rng) if k % 4 == 0 else interior(P, rng, 0.2)
            o = p - d * rng.uniform(0.1, 1.0) * ext / 4
            sc = 2.0 ** 40 if k % 8 < 4 else 2.0 ** -40
            R.add(o, d * sc, 0.0, "up" if sc > 1 else "down")
            continue
        # a first hit at distance D, with |dir| = D / t-max (1 +- 2^-e): t lands either side of t-max
        if len(P.small):
            _, c, r = P.pick_sphere(rng)
            u = unit(rng.normal(size=3))
            D = rng.uniform(0.02, 0.2) * r
            o, dd = c + u * (r + D), -u                       # straight at the sphere from just above it
        elif len(P.rects):
            ax, a0, a1, b0, b1, kk = P.rects[int(rng.integers(len(P.rects)))]
            D = rng.uniform(0.5, 5.0)
            dd = np.zeros(3)
            dd[RECT_AXES[ax][2]] = rng.choice([-1.0, 1.0])
            o = rect_point(ax, rng.uniform(a0, a1), rng.uniform(b0, b1), kk) - dd * D
        else:
            continue
        e = (10, 30, 45)[(k // 2) % 3]
        below = (k // 6) % 2 == 0
        # t = D / |dir|: a longer dir brings the hit below t-max
        R.add(o, dd * (D / TMAX * (1.0 + 2.0 ** -e if below else 1.0 - 2.0 ** -e)), 0.0,
              "tmax_below" if below else "tmax_above")
    return R.done()


def rays_time(P, rng, n=N):
    R = Rays()
    tlo, thi = P.times()
    t0, t1 = P.shutter
    mov = [i for i in P.small if P.moving[i] and P.t1[i] != P.t0[i]]
    for k in range(n):
        tm = (0.0, -0.0, t0, t1, 0.5 * (t0 + t1), None)[k % 6]
        tag = ("+0", "-0", "t0", "t1", "mid", "extrapolated")[k % 6]
        i = int(rng.choice(mov)) if mov and k % 3 != 2 else int(P.pick_sphere(rng)[0])
        if tm is None:                               # outside sphere i's own shutter, inside the trees' times
            a, b = min(P.t0[i], P.t1[i]), max(P.t0[i], P.t1[i])
            out = [(lo, hi) for lo, hi in ((tlo, min(a, thi)), (max(b, tlo), thi)) if hi > lo]
            if P.moving[i] and out:
                lo, hi = out[int(rng.integers(len(out)))]
                tm = float(rng.uniform(lo, hi))
            else:
                tm, tag = float(rng.uniform(tlo, thi)), "any"
        c = P.centre(i, tm)
        if not np.isfinite(c).all():
            c = P.centre(i, 0.0)
        r = P.r[i]
        d = rng.normal(size=3) if (k // 6) % 2 == 0 else escape_dir(P, rng)
        # through the sphere where it is at tm, or just past it (where it is at another time)
        u = perp(d, rng)
        u = u if u[1] >= 0 else -u
        off = u * r * (rng.uniform(0.0, 0.95) if (k // 12) % 2 == 0 else rng.uniform(1.05, 2.5))
        R.add(c + off - d * rng.uniform(1.5, 3.0) * r / np.linalg.norm(d), d, tm, tag)
    return R.done()


def rays_far(P, rng, n=N):
    R = Rays()
    ext = float(np.linalg.norm(P.hi - P.lo))
    for k in range(n):
        dist = P.radius * (1e6 if k % 2 == 0 else 1e9)
        u = unit(rng.normal(size=3))
        p = target(P, rng) if (k // 2) % 2 == 0 else interior(P, rng, 0.0) + unit(rng.normal(size=3)) * ext * 2
        o = p + u * dist
        d = unit(p - o) * (0.25, 0.9, 1.0, 3.0)[(k // 4) % 4]
        R.add(o, d, 0.0, "1e6" if k % 2 == 0 else "1e9")
    return R.done()


def rays_nonfinite(P, rng, n=12):
    R = Rays()
    bad = (np.nan, np.inf, -np.inf)
    for k in range(n):
        p = target(P, rng)
        d = rng.normal(size=3)
        o = p - d * 2.0
        if k % 2 == 0:
            d[k % 3] = bad[(k // 2) % 3]
        else:
            o[k % 3] = bad[(k // 2) % 3]
        R.add(o, d, 0.0, "dir" if k % 2 == 0 else "origin")
    return R.done()


_BUILDERS = {"axis": rays_axis, "plane": rays_plane, "tangent": rays_tangent, "surface": rays_surface,
             "inside": rays_inside, "scale": rays_scale, "time": rays_time, "far": rays_far,
             "nonfinite": rays_nonfinite}

_cache = {}


def scene_rays(name, make, classes):
    """(scene, {class: (rays (n, 7), tags)}) for a case: one seeded generator per (scene, class), cached."""
    key = (name, classes)
    if key not in _cache:
        sc = make(NX, NY)
        P = Prims(sc)
        out = {}
        for ci, cls in enumerate(CLASSES):
            if cls in classes:
                rng = np.random.default_rng([SEED, ci])
                with np.errstate(all="ignore"):
                    out[cls] = _BUILDERS[cls](P, rng)
        _cache[key] = (sc, out)
    return _cache[key]


def walk_rays(rays_by_class, walk):
    """The classes a walk takes: k_extend_lds's never sees a time but +0.0."""
    return {c: rt for c, rt in rays_by_class.items() if not (walk == WALK_LDS_TIME0 and c == "time")}


_flat = {}


def oracle_flat(oracle_mod, name, make, classes):
    """The flat-list truth of a case, computed once: {class: (t, mat)} with mat -1 and t 0 for a miss."""
    key = (name, classes)
    if key not in _flat:
        sc, rays = scene_rays(name, make, classes)
        o = oracle_mod.build_scene(sc)
        o.set_bvh_flat(True)
        _flat[key] = {c: oracle_hits(o, r) for c, (r, _) in rays.items()}
    return _flat[key]


def oracle_hits(o, rays):
    t = np.zeros(len(rays))
    m = np.full(len(rays), -1, dtype=np.int32)
    for k, r in enumerate(rays):
        h = o.hit_world(r[0:3], r[3:6], r[6])
        if h:
            t[k], m[k] = h[0], int(h[7])
    return t, m


def same_t(a, b):
    """Bit-for-bit equality of t arrays; two NaNs count as equal whatever their payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
