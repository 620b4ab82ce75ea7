"""Triangles and triangle meshes on the host: an OBJ reader, a few generators, and the NumPy restatement of
the rule include/rt.h states under "triangles" (the reference has no triangles, so that text is the rule).

The restatement — ``hit``, ``normal``, ``uv``, ``shading_normal`` — is written from the header alone: IEEE f64, the header's
operation order, no fused multiply-add (NumPy's elementwise arithmetic rounds every operation).  The GPU
tests compare librtamd's kernels against it bit for bit.
"""
import math

import numpy as np

TMIN = 0.001                 # main.scm:104
TMAX = 999999999999.0        # constant.scm:6


# ------------------------------------------------------------------ the rule
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def as_tris(vertices, faces=None):
    """(n, 3, 3) float64 triangles from (vertices, faces), or ``vertices`` itself if it already has that shape."""
    vs = np.asarray(vertices, dtype=np.float64)
    if faces is None:
        return vs.reshape(-1, 3, 3)
    return vs[np.asarray(faces, dtype=np.int64)]


def ray_constants(d):
    """The per-ray part of the test: (kx, ky, kz, Sx, Sy, Sz) for directions d (m, 3)."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    m = d.shape[0]
    rows = np.arange(m)
    ad = np.abs(d)
    kz = np.zeros(m, dtype=np.int64)
    kz[ad[:, 1] > ad[rows, kz]] = 1
    kz[ad[:, 2] > ad[rows, kz]] = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = d[rows, kz] < 0.0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        dz = d[rows, kz]
        return kx, ky, kz, d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz


def hit(tris, rays, tmin=TMIN, tmax=TMAX):
    """hit-obj-list over the triangles alone, in their order: for rays (m, >= 6) = origin, direction (already
    in the triangles' frame: see ``into_instance``) returns (t, index): the closest t in (tmin, tmax) and the
    triangle it belongs to — the first in list order among equals — or (0.0, -1) for a miss."""
    tris = as_tris(tris)
    r = np.asarray(rays, dtype=np.float64).reshape(-1, np.shape(rays)[-1])
    o, d = r[:, 0:3], r[:, 3:6]
    m = r.shape[0]
    rows = np.arange(m)
    kx, ky, kz, Sx, Sy, Sz = ray_constants(d)
    closest = np.full(m, float(tmax))
    best = np.full(m, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(tris.shape[0]):
            A, B, C = tris[i, 0] - o, tris[i, 1] - o, tris[i, 2] - o
            Az, Bz, Cz = A[rows, kz], B[rows, kz], C[rows, kz]
            Ax, Ay = A[rows, kx] - Sx * Az, A[rows, ky] - Sy * Az
            Bx, By = B[rows, kx] - Sx * Bz, B[rows, ky] - Sy * Bz
            Cx, Cy = C[rows, kx] - Sx * Cz, C[rows, ky] - Sy * Cz
            U = Cx * By - Cy * Bx
            V = Ax * Cy - Ay * Cx
            W = Bx * Ay - By * Ax
            miss = ((U < 0.0) | (V < 0.0) | (W < 0.0)) & ((U > 0.0) | (V > 0.0) | (W > 0.0))
            det = (U + V) + W
            miss |= det == 0.0
            T = (U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)
            t = T / det
            take = ~miss & (tmin < t) & (t < closest)          # (a NaN passes neither comparison)
            closest = np.where(take, t, closest)
            best = np.where(take, i, best)
    return np.where(best >= 0, closest, 0.0), best


def normal(tri):
    """The unit geometric normal of triangle(s) (..., 3, 3): n = cross(v1 - v0, v2 - v0) * (1 / sqrt(dot(n, n)))."""
    t = np.asarray(tri, dtype=np.float64)
    n = _cross(t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :])
    k = 1.0 / np.sqrt(_dot(n, n))
    return n * k[..., None]


def uv(tri, uvs, pt):
    """The hit record's (u, v) at point(s) pt (..., 3) of triangle tri (3, 3) with vertex texture coordinates
    uvs (3, 2) — or (0, 0) with uvs None."""
    pt = np.asarray(pt, dtype=np.float64)
    if uvs is None:
        z = np.zeros(pt.shape[:-1])
        return z, z.copy()
    t = np.asarray(tri, dtype=np.float64)
    q = np.asarray(uvs, dtype=np.float64)
    e1, e2 = t[1] - t[0], t[2] - t[0]
    n = _cross(e1, e2)
    w = pt - t[0]
    den = _dot(n, n)
    b1 = _dot(_cross(w, np.broadcast_to(e2, w.shape)), n) / den
    b2 = _dot(_cross(np.broadcast_to(e1, w.shape), w), n) / den
    b0 = (1.0 - b1) - b2
    return (b0 * q[0, 0] + b1 * q[1, 0]) + b2 * q[2, 0], (b0 * q[0, 1] + b1 * q[1, 1]) + b2 * q[2, 1]


def barycentrics(tri, pt):
    """(b1, b2) of point(s) pt (..., 3) on triangle tri (3, 3), as ``uv`` and ``shading_normal`` form them."""
    pt = np.asarray(pt, dtype=np.float64)
    t = np.asarray(tri, dtype=np.float64)
    e1, e2 = t[1] - t[0], t[2] - t[0]
    n = _cross(e1, e2)
    w = pt - t[0]
    den = _dot(n, n)
    b1 = _dot(_cross(w, np.broadcast_to(e2, w.shape)), n) / den
    b2 = _dot(_cross(np.broadcast_to(e1, w.shape), w), n) / den
    return b1, b2


def unit_normals(normals):
    """Vertex normals (..., 3) made unit as the add call makes them: n * (1.0 / sqrt(dot(n, n)))."""
    n = np.asarray(normals, dtype=np.float64)
    with np.errstate(all="ignore"):
        return n * (1.0 / np.sqrt(_dot(n, n)))[..., None]


def shading_normal(tri, vertex_normals, pt):
    """The hit record's normal at point(s) pt (..., 3) of triangle tri (3, 3) with vertex normals
    vertex_normals (3, 3) (made unit here as the add call makes them): s = (n0 + (n1 - n0) b1) + (n2 - n0) b2,
    q = dot(s, s), s * (1 / sqrt(q)) where q > 0 and finite, else the geometric normal."""
    pt = np.asarray(pt, dtype=np.float64)
    nk = unit_normals(np.asarray(vertex_normals, dtype=np.float64).reshape(3, 3))
    with np.errstate(all="ignore"):
        b1, b2 = barycentrics(tri, pt)
        s = (nk[0] + (nk[1] - nk[0]) * b1[..., None]) + (nk[2] - nk[0]) * b2[..., None]
        q = _dot(s, s)
        ok = (q > 0.0) & np.isfinite(q)
        out = s * (1.0 / np.sqrt(q))[..., None]
    return np.where(ok[..., None], out, np.broadcast_to(normal(tri), s.shape))


def vertex_normals(vertices, faces, weights="max"):
    """One unit normal per vertex: the unit normals of the faces around it, weighted, summed and made unit.
    weights="max" (the default): sin(angle) / (|a| |b|) for the face's angle at the vertex between its edges a
    and b there (N. Max, "Weights for computing vertex normals from facet normals", 1999), which gives the
    radial normal exactly for vertices on a sphere, whatever the faces' shapes (4e-16 on icosphere(2));
    weights="angle": the angle itself, which is off the radial direction by 8.9e-3 on icosphere(2) and 4.6e-3 on
    icosphere(3), where the midpoint subdivision leaves unequal faces around a vertex.
    A vertex no face uses gets (0, 0, 1)."""
    if weights not in ("max", "angle"):
        raise ValueError("vertex_normals: weights must be 'max' or 'angle'")
    vs = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    fs = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    t = vs[fs]
    fn = normal(t)
    acc = np.zeros_like(vs)
    for k in range(3):
        a = t[:, (k + 1) % 3] - t[:, k]
        b = t[:, (k + 2) % 3] - t[:, k]
        la, lb = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b))
        if weights == "angle":
            w = np.arccos(np.clip(_dot(a, b) / (la * lb), -1.0, 1.0))
        else:
            c = _cross(a, b)
            w = (np.sqrt(_dot(c, c)) / (la * lb)) / (la * lb)
        np.add.at(acc, fs[:, k], fn * w[:, None])
    ln = np.sqrt(_dot(acc, acc))
    acc[~(ln > 0.0)] = (0.0, 0.0, 1.0)
    return unit_normals(acc)


def radial_normals(vertices, center=(0.0, 0.0, 0.0)):
    """Unit normals pointing from ``center`` to each vertex: a sphere's normals at the vertices of its mesh."""
    vs = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return unit_normals(vs - np.asarray(center, dtype=np.float64))


def check_normals(normals, faces, who="mesh"):
    """What rt_add_mesh_normals refuses of the normals, as a ValueError: a normal of a face's vertex that is not
    finite, or whose length is zero or not finite."""
    ns = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    fs = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if fs.size and (fs.min() < 0 or fs.max() >= ns.shape[0]):
        raise ValueError("%s: a face index is out of range (%d normals)" % (who, ns.shape[0]))
    fin = np.isfinite(ns).all(axis=1)
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(ns, ns))
    good = fin & (ln > 0.0) & np.isfinite(ln)
    bad = np.nonzero(~good[fs].all(axis=1))[0]
    if bad.size:
        f = int(bad[0])
        what = "is not finite" if not fin[fs[f]].all() else "has zero or non-finite length"
        raise ValueError("%s: face %d has a vertex normal that %s" % (who, f, what))


def into_instance(rays, ops):
    """Rays (m, >= 6) taken into an instance chain: ops = [("translate", (x, y, z)) | ("rotate_y", degrees), ...],
    outermost first (g.translate(g.rotate_y(obj, a), off) is [("translate", off), ("rotate_y", a)])."""
    r = np.array(rays, dtype=np.float64)
    for kind, arg in ops:
        if kind == "translate":
            r[:, 0] = r[:, 0] - float(arg[0]); r[:, 1] = r[:, 1] - float(arg[1]); r[:, 2] = r[:, 2] - float(arg[2])
        elif kind == "rotate_y":
            rad = (math.pi / 180.0) * float(arg)               # geometry.scm:484
            sn, cs = math.sin(rad), math.cos(rad)
            for b in (0, 3):
                x, z = r[:, b].copy(), r[:, b + 2].copy()
                r[:, b] = cs * x - sn * z
                r[:, b + 2] = sn * x + cs * z
        else:
            raise ValueError(kind)
    return r


def out_of_instance(vec, ops, point=False):
    """Normal(s) (or, with point=True, point(s)) (..., 3) taken back out of the chain, innermost op first."""
    p = np.array(vec, dtype=np.float64)
    for kind, arg in reversed(list(ops)):
        if kind == "translate":
            if point:
                p = p + np.array([float(a) for a in arg])
        else:
            rad = (math.pi / 180.0) * float(arg)
            sn, cs = math.sin(rad), math.cos(rad)
            x, z = p[..., 0].copy(), p[..., 2].copy()
            p[..., 0] = cs * x + sn * z
            p[..., 2] = (-sn) * x + cs * z
    return p


def check_triangles(vertices, faces, who="mesh"):
    """What rt_add_triangle / rt_add_mesh refuse, as a ValueError: a vertex that is not finite, a face index out
    of range, a triangle whose cross(e1, e2) has zero or non-finite length."""
    vs = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    fs = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not np.isfinite(vs).all():
        raise ValueError("%s: a vertex is not finite" % who)
    if fs.size and (fs.min() < 0 or fs.max() >= vs.shape[0]):
        raise ValueError("%s: a face index is out of range (%d vertices)" % (who, vs.shape[0]))
    t = vs[fs]
    with np.errstate(all="ignore"):
        n = _cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        ln = np.sqrt(_dot(n, n))
    bad = np.nonzero(~(ln > 0.0) | ~np.isfinite(ln))[0]
    if bad.size:
        raise ValueError("%s: face %d is degenerate (cross(e1, e2) has zero or non-finite length)" % (who, int(bad[0])))


# ---------------------------------------------------------------- generators
def quad(p0, p1, p2, p3):
    """The quad p0 p1 p2 p3 as two triangles (0 1 2), (0 2 3) sharing the diagonal p0 p2; uvs (0,0) (1,0) (1,1) (0,1).
    Returns (vertices, faces, uvs)."""
    vs = np.array([p0, p1, p2, p3], dtype=np.float64)
    return vs, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64)


def rect_quad(axis, a0, a1, b0, b1, k, flip=False):
    """An axis rect (scene.make_xy_rect / xz / yz: axis 0 / 1 / 2) as a quad whose geometric normal is the
    rect's (+z / +y / +x, negated with flip) and whose uvs are the rect's u, v at the corners."""
    ia, ib = (1 if axis == 2 else 0), (1 if axis == 0 else 2)
    ik = 3 - ia - ib
    pts = []
    for a, b in ((a0, b0), (a1, b0), (a1, b1), (a0, b1)):
        p = [0.0, 0.0, 0.0]
        p[ia], p[ib], p[ik] = float(a), float(b), float(k)
        pts.append(p)
    vs, fs, uvs = quad(*pts)
    sign = normal(vs[fs[0]])[ik]
    if (sign < 0) != bool(flip):
        fs = fs[:, ::-1].copy()
    return vs, np.ascontiguousarray(fs, dtype=np.int32), uvs


def box(p0, p1):
    """g:make-box's six faces (geometry.scm:444-463, in its order: +z, -z, +y, -y, +x, -x) as 12 triangles over
    24 vertices, normals outward.  Returns (vertices, faces, uvs)."""
    faces = [(0, p0[0], p1[0], p0[1], p1[1], p1[2], False), (0, p0[0], p1[0], p0[1], p1[1], p0[2], True),
             (1, p0[0], p1[0], p0[2], p1[2], p1[1], False), (1, p0[0], p1[0], p0[2], p1[2], p0[1], True),
             (2, p0[1], p1[1], p0[2], p1[2], p1[0], False), (2, p0[1], p1[1], p0[2], p1[2], p0[0], True)]
    return merge([rect_quad(*f) for f in faces])


def merge(parts):
    """Several (vertices, faces, uvs) as one, in order."""
    vs, fs, us, base = [], [], [], 0
    for v, f, u in parts:
        vs.append(np.asarray(v, dtype=np.float64))
        fs.append(np.asarray(f, dtype=np.int32) + base)
        us.append(u)
        base += vs[-1].shape[0]
    uvs = None if any(u is None for u in us) else np.concatenate(us)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), uvs


def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """An icosahedron subdivided ``level`` times (20 * 4**level faces), vertices pushed to the sphere, normals
    outward.  Faces share vertices by index, so a shared edge has bit-identical end points in both.
    Returns (vertices, faces)."""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    vs = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
          (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    fs = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
          (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
          (8, 6, 7), (9, 8, 1)]

    def on_sphere(q):
        ln = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        return (q[0] / ln, q[1] / ln, q[2] / ln)

    vs = [on_sphere(q) for q in vs]
    for _ in range(int(level)):
        mid = {}

        def midpoint(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in mid:
                vs.append(on_sphere(tuple(0.5 * (vs[a][k] + vs[b][k]) for k in range(3))))
                mid[key] = len(vs) - 1
            return mid[key]

        nxt = []
        for a, b, c in fs:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        fs = nxt
    out = np.array(vs, dtype=np.float64) * float(radius) + np.array(center, dtype=np.float64)
    return out, np.array(fs, dtype=np.int32)


# ------------------------------------------------------------------ OBJ files
def read_obj(path, normals=False):
    """A Wavefront OBJ file's ``v``, ``vt``, ``vn`` and ``f`` lines (everything else is skipped): polygons are
    fanned from their first corner, indices may be negative (relative to the lines read so far), corners may be
    ``v``, ``v/vt``, ``v//vn`` or ``v/vt/vn`` (``vn`` is read with normals=True only).
    Returns (vertices (nv, 3), faces (nf, 3) int32, uvs (nv, 2) or None), and with normals=True a fourth entry,
    normals (nv, 3) or None.  OBJ indexes positions, texture coordinates and normals separately; a position
    used with several texture coordinates (with normals=True: or several normals) becomes several vertices.
    uvs is None unless every corner of every face names a ``vt``, normals likewise for ``vn``."""
    pos, tex, nor, corners, faces = [], [], [], {}, []
    verts, uvs, nrms = [], [], []
    all_vt = all_vn = True

    def index(tok, n, what, line_no):
        i = int(tok)
        i = i - 1 if i > 0 else n + i
        if i < 0 or i >= n or int(tok) == 0:
            raise ValueError("%s:%d: %s index %s out of range" % (path, line_no, what, tok))
        return i

    with open(path) as fh:
        for line_no, line in enumerate(fh, 1):
            w = line.split("#")[0].split()
            if not w:
                continue
            if w[0] == "v":
                pos.append(tuple(float(x) for x in w[1:4]))
            elif w[0] == "vt":
                tex.append((float(w[1]), float(w[2]) if len(w) > 2 else 0.0))
            elif w[0] == "vn" and normals:
                nor.append(tuple(float(x) for x in w[1:4]))
            elif w[0] == "f":
                ids = []
                for tok in w[1:]:
                    parts = tok.split("/")
                    vi = index(parts[0], len(pos), "vertex", line_no)
                    ti = index(parts[1], len(tex), "texture", line_no) if len(parts) > 1 and parts[1] else -1
                    ni = -1
                    if normals and len(parts) > 2 and parts[2]:
                        ni = index(parts[2], len(nor), "normal", line_no)
                    all_vt = all_vt and ti >= 0
                    all_vn = all_vn and ni >= 0
                    key = (vi, ti, ni) if normals else (vi, ti)
                    if key not in corners:
                        corners[key] = len(verts)
                        verts.append(pos[vi])
                        uvs.append(tex[ti] if ti >= 0 else (0.0, 0.0))
                        nrms.append(nor[ni] if ni >= 0 else (0.0, 0.0, 0.0))
                    ids.append(corners[key])
                if len(ids) < 3:
                    raise ValueError("%s:%d: a face needs at least 3 corners" % (path, line_no))
                for k in range(1, len(ids) - 1):
                    faces.append((ids[0], ids[k], ids[k + 1]))
    vs = np.array(verts, dtype=np.float64).reshape(-1, 3)
    fs = np.array(faces, dtype=np.int32).reshape(-1, 3)
    us = np.array(uvs, dtype=np.float64).reshape(-1, 2) if all_vt and len(faces) else None
    if not normals:
        return vs, fs, us
    return vs, fs, us, (np.array(nrms, dtype=np.float64).reshape(-1, 3) if all_vn and len(faces) else None)
