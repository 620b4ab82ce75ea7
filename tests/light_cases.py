"""Scenes, points and directions of the light-list tests (include/rt.h, "light lists"): shared by
test_light_list_host.py (NumPy restatement against the oracle and against itself) and test_gpu_light_list.py
(rt_light_probe and renders against the restatement)."""
import functools

import numpy as np

from rtamd import lights, mesh, scenes
from rtamd import scene as g
from rtamd.camera import make_camera

SEED = 0x5EED0701
NX = NY = 48
LAMP = (1, 213.0, 343.0, 227.0, 332.0, 554.0)            # cornell-box's ceiling light: axis, a0, a1, b0, b1, k


def _emit():
    return g.make_diffuse_light(g.constant_texture((3, 3, 3)))


def lamp_rect():
    """cornell_mixture's light, as the scene holds it (flipped)."""
    return g.flip_normals(g.make_xz_rect(213, 343, 227, 332, 554, _emit()))


def lamp_triangles():
    """The same rect as [t0, t1]: mesh.rect_quad's two triangles, which share the diagonal."""
    vs, fs, _ = mesh.rect_quad(1, 213, 343, 227, 332, 554, True)
    m = _emit()
    return [g.make_triangle(vs[f[0]], vs[f[1]], vs[f[2]], m) for f in fs]


def lamp_halves():
    m = _emit()
    return [g.flip_normals(g.make_xz_rect(213, 278, 227, 332, 554, m)), g.flip_normals(g.make_xz_rect(278, 343, 227, 332, 554, m))]


def sphere_light():
    """test_light_sampling.py's sphere."""
    return g.make_sphere((0, 3, 0), 0.7, g.make_diffuse_light(g.constant_texture((4, 4, 4))))


def sphere_scene(**kw):
    """test_light_sampling.py's sphere-light scene; kw: light=True or lights=True picks the keyword."""
    lam = g.make_lambertian(g.constant_texture((0.5, 0.5, 0.5)))
    light = sphere_light()
    cam = make_camera((0, 1, 5), (0, 1, 0), (0, 1, 0), 40, 1, 0, 1, 0, 1)
    extra = {"lights": [light]} if kw.get("lights") else {"light": light}
    return g.make_scene([g.make_sphere((0, -1000, 0), 1000, lam), light], cam, g.black, **extra)


def room(light=None, lights=None):
    """cornell-box's own objects with the given sampling; the geometry never changes."""
    sc = scenes.cornell_box(NX, NY)
    if light == "own":
        light = sc.obj_list[2]
    return g.make_scene(sc.obj_list, sc.camera, sc.sky_function, light=light, lights=lights)


def mixed_lights():
    """25 lights: a flipped xz rect, a sphere, a triangle, an xy rect, a yz rect, and icosphere(0) as a mesh."""
    m = _emit()
    vs, fs = mesh.icosphere(0, radius=40.0, center=(400.0, 300.0, 150.0))
    return [lamp_rect(), g.make_sphere((190, 90, 190), 90, m),
            g.make_triangle((100, 400, 100), (180, 420, 130), (120, 380, 220), m),
            g.make_xy_rect(50, 150, 200, 300, 500, m), g.make_yz_rect(100, 200, 300, 450, 20, m),
            g.make_mesh(vs, fs, m)]


PROBE_LISTS = {
    "rect": lambda: [lamp_rect()],
    "sphere": lambda: [g.make_sphere((190, 90, 190), 90, _emit())],
    "tri": lambda: [lamp_triangles()[0]],
    "two_tris": lamp_triangles,
    "mixed": mixed_lights,
}
HAS_SPHERE = {"sphere", "mixed"}


@functools.lru_cache(maxsize=None)
def probe_scene(name):
    """A small world (the lights need not be in it) whose light list is PROBE_LISTS[name]."""
    lam = g.make_lambertian(g.constant_texture((0.5, 0.5, 0.5)))
    cam = make_camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40, 1, 0, 10, 0, 1)
    return g.make_scene([g.make_sphere((278, -1000, 278), 1000, lam)], cam, g.black, lights=PROBE_LISTS[name]())


def _targets(flat, rs, n):
    """n points on and around the lights: vertices, points of edges (a quad's shared diagonal among them),
    interior points, and points a little off."""
    out = []
    for L in flat:
        if L[0] == "tri":
            t = L[1]
            out += [t[0], t[1], t[2]]
            for a, b in ((0, 1), (1, 2), (2, 0)):
                for u in rs.random(3):
                    out.append(t[a] + (t[b] - t[a]) * u)
            for _ in range(6):
                b1, b2 = np.sort(rs.random(2))
                out.append(t[0] * b1 + t[1] * (b2 - b1) + t[2] * (1 - b2))
        elif L[0] == "rect":
            _, axis, a0, a1, b0, b1, k = L
            ia, ib, ik = lights._AXES[axis]
            for a, b in [(a0, b0), (a1, b0), (a1, b1), (a0, b1), (a0, 0.5 * (b0 + b1))] + \
                    [(a0 + (a1 - a0) * rs.random(), b0 + (b1 - b0) * rs.random()) for _ in range(8)]:
                p = np.zeros(3)
                p[ia], p[ib], p[ik] = a, b, k
                out.append(p)
        else:
            _, c, r = L
            for _ in range(12):
                d = rs.normal(size=3)
                out.append(c + d / np.linalg.norm(d) * r * rs.choice([0.5, 1.0, 1.05]))
    out = np.array(out)
    pick = out[rs.randint(0, len(out), n)]
    jitter = np.where(rs.random((n, 1)) < 0.5, 0.0, rs.normal(size=(n, 3)) * 5.0)     # half exactly at, half around
    return pick + jitter


@functools.lru_cache(maxsize=None)
def probe_points(name):
    """(points (n, 3), dirs (n, 3)) for PROBE_LISTS[name]: 1024 random points, points in a light's plane,
    points inside a sphere light; directions at and around the lights (edges and vertices exactly), axis-parallel,
    zero and non-finite ones."""
    flat = lights.flatten(PROBE_LISTS[name]())
    rs = np.random.RandomState((SEED + sorted(PROBE_LISTS).index(name)) & 0x7FFFFFFF)
    pts = [rs.random((1024, 3)) * np.array([555.0, 540.0, 555.0])]
    for L in flat[:6]:
        if L[0] == "rect":                                   # in the rect's plane
            _, axis, a0, a1, b0, b1, k = L
            p = rs.random((16, 3)) * 555.0
            p[:, lights._AXES[axis][2]] = k
            pts.append(p)
        elif L[0] == "tri":                                  # in the triangle's plane (as nearly as f64 puts them)
            t = L[1]
            w = rs.random((16, 2)) * 3.0 - 1.0
            pts.append(t[0] + (t[1] - t[0]) * w[:, :1] + (t[2] - t[0]) * w[:, 1:])
        else:                                                # inside the sphere
            _, c, r = L
            d = rs.normal(size=(16, 3))
            pts.append(c + d / np.linalg.norm(d, axis=1, keepdims=True) * r * rs.random((16, 1)) * 0.9)
    pts = np.concatenate(pts)
    n = len(pts)
    dirs = _targets(flat, rs, n) - pts
    k = np.arange(n)
    axis_par = np.eye(3)[k % 3] * np.where((k // 3) % 2 == 0, 1.0, -1.0)[:, None] * 2.5
    dirs = np.where((k % 8 == 5)[:, None], axis_par, dirs)
    dirs = np.where((k % 64 == 6)[:, None], 0.0, dirs)
    bad = np.array([[np.nan, 1.0, 0.0], [np.inf, 0.0, 1.0], [0.0, -np.inf, 0.0], [1.0, 1.0, np.nan]])
    dirs = np.where((k % 64 == 7)[:, None], bad[(k // 64) % 4], dirs)
    return np.ascontiguousarray(pts), np.ascontiguousarray(dirs)


def clamped_moments(render_pass, passes):
    """ΣA and ΣA² over `passes` one-pass renders, A = the mean over channels of min(x, 1.0) per pixel;
    render_pass(k) returns pass k's nx*ny*3 samples."""
    S = np.zeros(NX * NY)
    Q = np.zeros(NX * NY)
    for k in range(passes):
        a = np.minimum(render_pass(k).reshape(-1, 3), 1.0).mean(axis=1)
        S += a
        Q += a * a
    return S, Q


def mean_and_var(S, Q, passes):
    """The frame mean of A and the variance of that mean (test_gpu_triangles.py's mean_and_var, over every pixel)."""
    m = S / passes
    var_mean = (Q / passes - m * m) * (passes / (passes - 1.0)) / passes
    return float(m.mean()), float(var_mean.sum() / m.size ** 2)
