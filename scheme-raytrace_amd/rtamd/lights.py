"""Light lists on the host: the NumPy restatement of the rule include/rt.h states under "light lists" — the
density and the sampler of the mixture's light side over a list of rects, spheres and triangles.

Written from the header text: IEEE f64, the header's operation order, no fused multiply-add.  ``pdf_value`` is
vectorised over rays; ``random`` follows one path stream (rng.path_draw) and uses the C library's sin / cos, so
it states the RT_LIBM_EXACT mode of the sphere sampler.  The triangle test is rtamd.mesh.hit.  The GPU tests
compare rt_light_probe against these bit for bit.
"""
import math

import numpy as np

from . import mesh, rng
from ._lib import RT_MAX_LIGHTS

TMIN, TMAX = mesh.TMIN, mesh.TMAX


class Light(tuple):
    """One flattened light: ("rect", axis, a0, a1, b0, b1, k) | ("sphere", centre (3,), r) | ("tri", (3, 3))."""
    __slots__ = ()


def flatten(objs):
    """rt_set_light_list's flattening of scene descriptors (rects, spheres, triangles, flips of these, meshes;
    Light records pass through), in order.  ValueError for what the ABI refuses, and for an empty result."""
    out = []

    def walk(o):
        if isinstance(o, Light):
            out.append(o)
            return
        kind = getattr(o, "kind", None)
        a = getattr(o, "args", ())
        if kind == "flip":
            walk(a[0])                            # a flip does not change sampling
        elif kind == "rect":
            out.append(Light(("rect", int(a[0])) + tuple(float(x) for x in a[1:6])))
        elif kind == "sphere":
            out.append(Light(("sphere", np.array([float(x) for x in a[0]]), float(a[1]))))
        elif kind == "triangle":
            out.append(Light(("tri", np.array([[float(x) for x in p] for p in a[0:3]]))))
        elif kind == "mesh":
            for t in mesh.as_tris(a[0], a[1]):
                out.append(Light(("tri", np.array(t, dtype=np.float64))))
        else:
            raise ValueError("a light must be a rect, a sphere or a triangle (optionally flipped) or a mesh, not %r" % (o,))

    for o in objs:
        walk(o)
    if not out:
        raise ValueError("the light list holds no light")
    if len(out) > RT_MAX_LIGHTS:
        raise ValueError("more than RT_MAX_LIGHTS (%d) lights" % RT_MAX_LIGHTS)
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


_AXES = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}       # rect axis -> (a, b, k) components


def _rect_pdf(L, o, v):
    _, axis, a0, a1, b0, b1, k = L
    ia, ib, ik = _AXES[axis]
    n = np.zeros(3)
    n[ik] = 1.0
    t = (k - o[:, ik]) / v[:, ik]
    miss = (t < TMIN) | (t > TMAX)                          # (a NaN passes on, as in the kernels)
    A, B = o[:, ia] + t * v[:, ia], o[:, ib] + t * v[:, ib]
    miss |= (A < a0) | (A > a1) | (B < b0) | (B > b1)
    area = (a1 - a0) * (b1 - b0)
    vv = _dot(v, v)
    distance_squared = t * t * vv
    cosine = np.abs(_dot(v, np.broadcast_to(n, v.shape)) / np.sqrt(vv))
    return np.where(miss, 0.0, distance_squared / (cosine * area))


def _sphere_pdf(L, o, v):
    _, c, r = L
    oc = o - c
    a, b, cc = _dot(v, v), _dot(oc, v), _dot(oc, oc) - r * r
    disc = b * b - a * cc
    miss = disc <= 0.0
    sq = np.sqrt(disc)
    t1, t2 = (-b - sq) / a, (-b + sq) / a
    hit = ((TMIN < t1) & (t1 < TMAX)) | ((TMIN < t2) & (t2 < TMAX))
    co = c - o
    cos_theta_max = np.sqrt(1.0 - r * r / _dot(co, co))
    solid_angle = 2.0 * math.pi * (1.0 - cos_theta_max)
    return np.where(~miss & hit, 1.0 / solid_angle, 0.0)


def tri_area_normal(tri):
    """(area, unit normal) of a triangle (3, 3), as the commit forms them."""
    n = mesh._cross(tri[1] - tri[0], tri[2] - tri[0])
    return 0.5 * np.sqrt(_dot(n, n)), mesh.normal(tri)


def _tri_pdf(L, o, v):
    tri = L[1]
    area, nu = tri_area_normal(tri)
    t, idx = mesh.hit(tri[None], np.concatenate([o, v], axis=1), TMIN, TMAX)
    vv = _dot(v, v)
    distance_squared = (t * t) * vv
    cosine = np.abs(_dot(v, np.broadcast_to(nu, v.shape)) / np.sqrt(vv))
    return np.where(idx >= 0, distance_squared / (cosine * area), 0.0)


_PDF = {"rect": _rect_pdf, "sphere": _sphere_pdf, "tri": _tri_pdf}


def pdf_value(lights, o, v):
    """pdf_value(o, v) of the list for rays (o, v): v (n, 3), o (3,) or (n, 3).  Returns (n,) float64."""
    ls = flatten(lights)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, dtype=np.float64), v.shape))
    w = 1.0 / float(len(ls))
    s = np.zeros(v.shape[0])
    with np.errstate(all="ignore"):
        for L in ls:
            s = s + w * _PDF[L[0]](L, o, v)
    return s


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")


def _unit(a):
    ln = _sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    k = 1.0 / ln if ln != 0.0 else float("inf")
    return (a[0] * k, a[1] * k, a[2] * k)


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def random(lights, o, seed, pix):
    """random(o) of the list on the path stream (seed, pixel pix, sample 0) from its first number.
    Returns (direction (3,) float64, draws)."""
    ls = flatten(lights)
    o = [float(x) for x in o]
    ctr = [0]

    def nxt():
        u = rng.path_draw(seed, pix, 0, ctr[0])
        ctr[0] += 1
        return u

    m = len(ls)
    i = 0
    if m > 1:
        r = nxt()
        i = int(r * float(m))
        if i > m - 1:
            i = m - 1
    L = ls[i]
    if L[0] == "rect":
        _, axis, a0, a1, b0, b1, k = L
        a = a0 + nxt() * (a1 - a0)
        b = b0 + nxt() * (b1 - b0)
        ia, ib, ik = _AXES[axis]
        pnt = [0.0, 0.0, 0.0]
        pnt[ia], pnt[ib], pnt[ik] = a, b, k
        d = (pnt[0] - o[0], pnt[1] - o[1], pnt[2] - o[2])
    elif L[0] == "tri":
        v0, v1, v2 = [[float(x) for x in p] for p in L[1]]
        r1 = nxt()
        r2 = nxt()
        su = math.sqrt(r1)
        b1, b2 = su * (1.0 - r2), su * r2
        d = tuple((v0[k] + ((v1[k] - v0[k]) * b1 + (v2[k] - v0[k]) * b2)) - o[k] for k in range(3))
    else:
        _, c, radius = L
        direction = (float(c[0]) - o[0], float(c[1]) - o[1], float(c[2]) - o[2])
        distance_squared = (direction[0] * direction[0] + direction[1] * direction[1]) + direction[2] * direction[2]
        w = _unit(direction)
        aa = (0.0, 1.0, 0.0) if abs(w[0]) > 0.9 else (1.0, 0.0, 0.0)
        vv = _unit(_cross(w, aa))
        uu = _cross(w, vv)

        def to_sphere():                          # random-to-sphere: evaluated three times, one component each
            r1 = nxt()
            r2 = nxt()
            z = 1.0 + r2 * (_sqrt(1.0 - radius * radius / distance_squared) - 1.0)
            phi = 2.0 * math.pi * r1
            s = _sqrt(1.0 - z * z)
            return (math.cos(phi) * s, math.sin(phi) * s, z)

        x = to_sphere()[0]
        y = to_sphere()[1]
        z = to_sphere()[2]
        d = tuple((uu[k] * x + vv[k] * y) + w[k] * z for k in range(3))
    return np.array(d, dtype=np.float64), ctr[0]
