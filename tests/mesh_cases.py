"""Shared by test_mesh_host.py and test_gpu_triangles.py: the triangle scenes, their probe rays, and the
expected closest hits built from rtamd.mesh (the NumPy restatement of include/rt.h's "triangles") merged with
the oracle's hit_world for the leaves the oracle can hold.  Every result is computed once per session."""
import functools

import numpy as np

import hit_ray_cases as hc
from rtamd import mesh
from rtamd import scene as g
from rtamd.camera import make_camera

SEED = 0x5EED0601
NX = NY = 48


def _cam():
    return make_camera((0, 1, 6), (0, 0, 0), (0, 1, 0), 40, 1.0, 0, 1, 0, 1)


def _mat(r, gr, b):
    return g.make_lambertian(g.constant_texture((r, gr, b)))


# ------------------------------------------------------------------ flattening
class Leaf:
    """One top-level object of a test scene: a group of triangles (tris, local frame) or another leaf."""
    def __init__(self, obj, ops, flip, pos):
        self.obj, self.ops, self.flip, self.pos = obj, ops, flip, pos
        self.tris = self.uvs = None
        if obj.kind == "triangle":
            self.tris = np.array([obj.args[0:3]], dtype=np.float64)
        elif obj.kind == "mesh":
            self.tris = mesh.as_tris(obj.args[0], obj.args[1])
            if obj.args[2] is not None:
                self.uvs = np.asarray(obj.args[2])[np.asarray(obj.args[1])]
        self.material = obj.args[-1] if self.tris is not None else None

    def world_tris(self):
        return mesh.out_of_instance(self.tris, self.ops, point=True)


def leaves_of(scene):
    """The scene's top-level objects, each walked through flip / translate / rotate_y down to its primitive."""
    out = []
    for pos, o in enumerate(scene.obj_list):
        ops, flip = [], False
        while o.kind in ("flip", "translate", "rotate_y"):
            if o.kind == "flip":
                flip = not flip
            else:
                ops.append((o.kind, o.args[1]))
            o = o.args[0]
        out.append(Leaf(o, ops, flip, pos))
    return out


class _MatIds:
    """A builder that only numbers materials as GpuBuilder / the oracle number them: in emission order."""
    def __init__(self):
        self.n = 0

    def __getattr__(self, name):
        if name.startswith("material_"):
            def f(*a):
                self.n += 1
                return self.n - 1
            return f
        return lambda *a: 0


def material_ids(scene):
    """{id(Material): material id} of the scene as emitted."""
    # emit numbers a material at its first use, objects in list order (each test object has one material)
    b, memo, n = _MatIds(), {}, 0
    g.emit(scene, b)
    for lf in leaves_of(scene):
        m = lf.obj.args[-1]
        if id(m) not in memo:
            memo[id(m)] = n
            n += 1
    assert n == b.n, (n, b.n)
    return memo


def without_triangles(scene):
    """The scene's other objects as a scene of their own (for the oracle), or None if there are none."""
    rest = [o for o, lf in zip(scene.obj_list, leaves_of(scene)) if lf.tris is None]
    return g.make_scene(rest, scene.camera, scene.sky_function) if rest else None


def expected_hits(oracle_mod, scene, rays):
    """(t, material id) of hit-obj-list over the scene: rtamd.mesh.hit over its triangles, in list order, merged
    with the oracle's hit_world over the rest.  A rect at the same t as a triangle wins; a sphere wins only
    if it is listed first; a rect's NaN t (a ray in its plane) wins as the list lets it (Q20)."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 7)
    ids = material_ids(scene)
    n = rays.shape[0]
    t = np.full(n, mesh.TMAX)
    mat = np.full(n, -1, dtype=np.int32)
    pos = np.full(n, -1)
    for lf in leaves_of(scene):
        if lf.tris is None:
            continue
        tt, idx = mesh.hit(lf.tris, mesh.into_instance(rays, lf.ops))
        take = (idx >= 0) & (tt < t)                               # (list order: the first at the smallest t)
        t = np.where(take, tt, t)
        mat = np.where(take, ids[id(lf.material)], mat).astype(np.int32)
        pos = np.where(take, lf.pos, pos)
    rest = without_triangles(scene)
    if rest is not None:
        o = oracle_mod.build_scene(rest)
        o.set_bvh_flat(True)
        to, mo = hc.oracle_hits(o, rays)
        rest_leaves = [lf for lf in leaves_of(scene) if lf.tris is None]
        rest_ids = material_ids(rest)
        back = {rest_ids[id(lf.obj.args[-1])]: lf for lf in rest_leaves}
        for k in range(n):
            if mo[k] < 0:
                continue
            lf = back[int(mo[k])]                                  # (the test scenes give every other leaf its own material)
            rect = lf.obj.kind == "rect"
            wins = np.isnan(to[k]) or mat[k] < 0 or to[k] < t[k] or (to[k] == t[k] and (rect or lf.pos < pos[k]))
            if wins:
                t[k], mat[k] = to[k], ids[id(lf.obj.args[-1])]
    return np.where(mat >= 0, t, 0.0), mat


# ---------------------------------------------------------------------- scenes
TRI = ((-1.0, -0.5, -1.0), (1.5, -0.25, -0.5), (0.25, 1.5, -1.75))          # one oblique triangle
QUAD = ((-1.0, -1.0, -1.0), (1.0, -1.0, -1.0), (1.0, 1.0, -1.0), (-1.0, 1.0, -1.0))   # in the plane z = -1


def one_triangle():
    return g.make_scene([g.make_triangle(*TRI, _mat(0.8, 0.2, 0.2))], _cam(), g.sky_color)


def quad_scene():
    vs, fs, uvs = mesh.quad(*QUAD)
    return g.make_scene([g.make_mesh(vs, fs, _mat(0.2, 0.8, 0.2), uvs)], _cam(), g.sky_color)


def coincident_triangles():
    a, b, c = QUAD[0], QUAD[1], QUAD[2]
    return g.make_scene([g.make_triangle(a, b, c, _mat(0.1, 0.1, 0.9)), g.make_triangle(a, b, c, _mat(0.9, 0.9, 0.1))],
                        _cam(), g.sky_color)


def _tri_and_rect(rect_first):
    vs, fs, _ = mesh.quad(*QUAD)
    tri = g.make_mesh(vs, fs, _mat(0.1, 0.5, 0.9))
    rect = g.make_xy_rect(-1.0, 1.0, -1.0, 1.0, -1.0, _mat(0.9, 0.5, 0.1))
    return g.make_scene([rect, tri] if rect_first else [tri, rect], _cam(), g.sky_color)


def rect_then_triangles():
    return _tri_and_rect(True)


def triangles_then_rect():
    return _tri_and_rect(False)


def ball_among_spheres():
    """icosphere(2) among 20 world-level spheres and 3 moving spheres (each with a material of its own)."""
    rng = np.random.RandomState(SEED & 0x7FFFFFFF)
    vs, fs = mesh.icosphere(2, radius=1.0, center=(0.0, 0.25, -0.5))
    objs = [g.make_mesh(vs, fs, _mat(0.7, 0.7, 0.7))]
    for k in range(23):
        c = rng.uniform(-4, 4, 3)
        c[1] = abs(c[1]) * 0.5
        m = _mat(*rng.uniform(0.1, 0.9, 3))
        r = float(rng.uniform(0.2, 0.6))
        if k < 20:
            objs.append(g.make_sphere(tuple(c), r, m))
        else:
            objs.append(g.make_moving_sphere(tuple(c), tuple(c + rng.uniform(-0.5, 0.5, 3)), 0.0, 1.0, r, m))
    return g.make_scene(objs, _cam(), g.sky_color)


def instanced_quad():
    vs, fs, uvs = mesh.quad(*QUAD)
    q = g.make_mesh(vs, fs, _mat(0.3, 0.3, 0.8), uvs)
    return g.make_scene([g.translate(g.rotate_y(g.flip_normals(q), 37.0), (0.5, 0.25, -1.0))], _cam(), g.sky_color)


SCENES = {"one_triangle": one_triangle, "quad": quad_scene, "coincident_triangles": coincident_triangles,
          "rect_then_triangles": rect_then_triangles, "triangles_then_rect": triangles_then_rect,
          "ball_among_spheres": ball_among_spheres, "instanced_quad": instanced_quad}
TRI_LEAVES = {"one_triangle": 1, "quad": 2, "coincident_triangles": 2, "rect_then_triangles": 2,
              "triangles_then_rect": 2, "ball_among_spheres": 320, "instanced_quad": 2}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name]()


# ------------------------------------------------------------------------ rays
def _edges(tris):
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    return e[:, 0], e[:, 1]


def _aimed(origins, targets, tm=0.0):
    o = np.repeat(origins, len(targets), axis=0)
    p = np.tile(targets, (len(origins), 1))
    return np.concatenate([o, p - o, np.full((len(o), 1), tm)], axis=1)


def probe_rays(name):
    """{class: rays (n, 7)} for a scene: the issue's ray classes, aimed at the scene's triangles in world space."""
    rng = np.random.RandomState((SEED + sorted(SCENES).index(name)) & 0x7FFFFFFF)
    T = np.concatenate([lf.world_tris() for lf in leaves_of(scene_of(name)) if lf.tris is not None])
    T = T[:: max(1, len(T) // 24)]                                 # (a ball: every 13th triangle is enough to aim at)
    cen = T.mean(axis=(0, 1))
    nrm = mesh.normal(T)
    a, b = _edges(T)
    origins = cen + nrm[0] * 3.0 + rng.uniform(-1.5, 1.5, (6, 3))
    out = {}
    f = rng.uniform(0.0, 1.0, (len(a), 1))
    out["edges_vertices"] = _aimed(origins, np.concatenate([T.reshape(-1, 3), 0.5 * (a + b), a + (b - a) * f]))
    # in the triangle's plane: origin and direction combinations of its edges (exact for the axis-aligned ones)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    rows = []
    for k in range(len(T)):
        for (oa, ob, da, db) in ((-0.5, 0.25, 1.0, 0.0), (0.25, 0.25, 0.5, 0.5), (2.0, 2.0, -1.0, -1.0), (0.5, -1.0, 0.0, 1.0)):
            rows.append(np.concatenate([T[k, 0] + oa * e1[k] + ob * e2[k], da * e1[k] + db * e2[k], [0.0]]))
    out["in_plane"] = np.array(rows)
    # parallel to an edge: off the plane, passing over the triangle
    rows = []
    for k in range(len(T)):
        for off in (0.5, -0.25, 0.0):
            o = T[k].mean(axis=0) + off * nrm[k] - 2.0 * e1[k]
            rows.append(np.concatenate([o, e1[k], [0.0]]))
    out["edge_parallel"] = np.array(rows)
    # axis-parallel, the six directions (a zero Sx or Sy; a negative d[kz]), through interior points, vertices and edges
    pts = np.concatenate([T.mean(axis=1), T[:, 0], 0.5 * (T[:, 0] + T[:, 1])])
    rows = []
    for ax in range(3):
        for sgn in (1.0, -1.0):
            d = np.zeros(3)
            d[ax] = sgn
            for p in pts:
                rows.append(np.concatenate([p - 2.5 * d, d * rng.choice([0.5, 1.0, 3.0]), [0.0]]))
    out["axis"] = np.array(rows)
    # two components of equal magnitude (the kz tie keeps the lower axis)
    rows = []
    for d in ((1, 1, 0.25), (-1, 1, 0.25), (1, -1, -0.5), (0.5, 2, 2), (0.5, -2, 2), (2, 0.5, -2), (-2, 0.5, -2), (1, 1, 1),
              (-1, -1, -1), (1, -1, 1), (3, 3, -3)):
        d = np.array(d, dtype=np.float64)
        for p in pts[:: max(1, len(pts) // 12)]:
            rows.append(np.concatenate([p - 1.75 * d, d, [0.0]]))
    out["equal_magnitude"] = np.array(rows)
    # origins a few ulps either side of t = 0.001 in front of the surface
    rows = []
    for k in range(len(T)):
        p = T[k].mean(axis=0)
        d = -nrm[k]
        o = p - d * 0.001
        for ulps in range(-4, 5):
            oo = o.copy()
            for _ in range(abs(ulps)):
                oo = np.nextafter(oo, oo + (np.sign(ulps) * d))
            rows.append(np.concatenate([oo, d, [0.0]]))
        ax = int(np.argmax(np.abs(nrm[k])))                        # and along an axis, where o + d * t is exact
        d = np.zeros(3)
        d[ax] = -np.sign(nrm[k][ax])
        for ulps in range(-4, 5):
            oo = p - d * 0.001
            for _ in range(abs(ulps)):
                oo[ax] = np.nextafter(oo[ax], oo[ax] + np.sign(ulps) * d[ax])
            rows.append(np.concatenate([oo, d, [0.0]]))
    out["tmin"] = np.array(rows)
    # components that are not finite
    base = np.concatenate([origins[0], cen - origins[0], [0.0]])
    rows = []
    for col in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[col] = bad
            rows.append(r)
    out["nonfinite"] = np.array(rows)
    # seeded random rays, most of them towards the scene
    o = rng.uniform(-5, 5, (4096, 3))
    tgt = cen + rng.uniform(-2.0, 2.0, (4096, 3))
    d = np.where(rng.uniform(size=(4096, 1)) < 0.8, tgt - o, rng.normal(size=(4096, 3)))
    out["random"] = np.concatenate([o, d, rng.uniform(0, 1, (4096, 1))], axis=1)
    return out


@functools.lru_cache(maxsize=None)
def _all_rays(name):
    by_class = probe_rays(name)
    names = sorted(by_class)
    rays = np.ascontiguousarray(np.concatenate([by_class[c] for c in names]))
    cls = np.concatenate([np.full(len(by_class[c]), i) for i, c in enumerate(names)])
    rays.setflags(write=False)
    return names, rays, cls


def scene_rays(name):
    """(class names, rays (n, 7) of all classes, class index per ray)."""
    return _all_rays(name)


_expected = {}


def expected(oracle_mod, name):
    if name not in _expected:
        t, m = expected_hits(oracle_mod, scene_of(name), _all_rays(name)[1])
        t.setflags(write=False)
        m.setflags(write=False)
        _expected[name] = (t, m)
    return _expected[name]


# --------------------------------------------------------------- watertightness
BALL_LEVEL = 2


@functools.lru_cache(maxsize=None)
def watertight_rays():
    """icosphere(2): from its centre and from 200 seeded interior points, rays aimed exactly at every vertex,
    every edge midpoint and a seeded point on every edge.  (rays (n, 7), vertices, faces)"""
    rng = np.random.RandomState((SEED ^ 0x77) & 0x7FFFFFFF)
    vs, fs = mesh.icosphere(BALL_LEVEL)
    e = np.unique(np.sort(np.concatenate([fs[:, [0, 1]], fs[:, [1, 2]], fs[:, [2, 0]]]), axis=1), axis=0)
    a, b = vs[e[:, 0]], vs[e[:, 1]]
    targets = np.concatenate([vs, 0.5 * (a + b), a + (b - a) * rng.uniform(0, 1, (len(e), 1))])
    inner = rng.normal(size=(200, 3))
    inner = inner / np.linalg.norm(inner, axis=1, keepdims=True) * rng.uniform(0.0, 0.6, (200, 1))
    rays = _aimed(np.concatenate([np.zeros((1, 3)), inner]), targets)
    rays.setflags(write=False)
    return rays, vs, fs


def moller_trumbore(tris, rays, tmin=mesh.TMIN, tmax=mesh.TMAX, eps=0.0):
    """The Möller–Trumbore test, restated for comparison only: (t, index) like mesh.hit."""
    tris = mesh.as_tris(tris)
    o, d = rays[:, 0:3], rays[:, 3:6]
    closest = np.full(len(rays), float(tmax))
    best = np.full(len(rays), -1)
    with np.errstate(all="ignore"):
        for i in range(len(tris)):
            e1, e2 = tris[i, 1] - tris[i, 0], tris[i, 2] - tris[i, 0]
            p = np.cross(d, e2)
            det = p @ e1
            inv = 1.0 / det
            s = o - tris[i, 0]
            u = np.einsum("ij,ij->i", s, p) * inv
            q = np.cross(s, e1)
            v = np.einsum("ij,ij->i", d, q) * inv
            t = (q @ e2) * inv
            take = (np.abs(det) > eps) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tmin < t) & (t < closest)
            closest = np.where(take, t, closest)
            best = np.where(take, i, best)
    return np.where(best >= 0, closest, 0.0), best
