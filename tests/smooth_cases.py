"""Shared by test_smooth_normals_host.py and test_gpu_smooth_normals.py: hit points on icospheres, the scenes with
smooth meshes, the expected first-hit features built from rtamd.mesh (hit, shading_normal), and ``scatter``:
the metal and dielectric steps restated from the oracle's exports as they stand (stream, reflect, refract,
schlick) and rtamd.vec, so that a scatter from a shading normal the oracle cannot hold has an expectation."""
import functools
import math

import numpy as np

import feature_cases as fc
import mesh_cases as mc
from rtamd import mesh
from rtamd import scene as g
from rtamd import vec as v
from rtamd.camera import make_camera

SEED = 0x5EED0701
SMP = 2
NX = NY = 48
KMAX = 100                       # kMaxDepth (rt_device.h), ORC_MAX_DEPTH


def _lam(r, gr, b):
    return g.make_lambertian(g.constant_texture((r, gr, b)))


# ------------------------------------------------------------------ sphere hits
@functools.lru_cache(maxsize=None)
def sphere_hits(level, n=6000, radius=90.0, center=(190.0, 91.0, 190.0), seed=1):
    """Camera-like rays onto icosphere(level): from seeded origins 4 to 8 radii away, aimed at seeded points
    inside the ball.  Returns (vertices, faces, hit points (m, 3) in the mesh's frame, face index (m,)) of the
    rays that hit (all do: the targets are inside the inscribed sphere)."""
    rng = np.random.RandomState(seed)
    c = np.array(center)
    vs, fs = mesh.icosphere(level, radius, center)
    d = rng.normal(size=(n, 3))
    o = c + d / np.linalg.norm(d, axis=1, keepdims=True) * radius * rng.uniform(4.0, 8.0, (n, 1))
    tgt = rng.normal(size=(n, 3))
    tgt = c + tgt / np.linalg.norm(tgt, axis=1, keepdims=True) * radius * 0.7 * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)
    rays = np.concatenate([o, tgt - o, np.zeros((n, 1))], axis=1)
    t, idx = mesh.hit(vs[fs], rays)
    ok = idx >= 0
    pt = rays[ok, 0:3] + rays[ok, 3:6] * t[ok, None]
    for a in (vs, fs, pt):
        a.setflags(write=False)
    return vs, fs, pt, idx[ok]


def shading_normals_at(vs, fs, normals, pt, idx):
    """mesh.shading_normal at points pt of faces idx, face by face."""
    out = np.zeros_like(pt)
    tris = vs[fs]
    for f in np.unique(idx):
        sel = idx == f
        out[sel] = mesh.shading_normal(tris[f], normals[fs[f]], pt[sel])
    return out


# ---------------------------------------------------------------------- scenes
CHAIN = (37.0, (0.5, 0.25, -1.0))            # rotate-y degrees, then translate (mesh_cases.instanced_quad's)


@functools.lru_cache(maxsize=None)
def flipped_ball_scene():
    """icosphere(1) with radial normals under flip + rotate-y 37 + translate, beside a plain (flat) quad."""
    vs, fs = mesh.icosphere(1, radius=1.0, center=(0.0, 0.25, 0.0))
    ball = g.make_mesh(vs, fs, _lam(0.7, 0.4, 0.2), normals=mesh.radial_normals(vs, (0.0, 0.25, 0.0)))
    qv, qf, _ = mesh.quad((-3.0, -1.0, -2.5), (-1.0, -1.0, -2.0), (-1.0, 1.0, -2.0), (-3.0, 1.0, -2.5))
    quad = g.make_mesh(qv, qf, _lam(0.2, 0.3, 0.8))
    return g.make_scene([g.translate(g.rotate_y(g.flip_normals(ball), CHAIN[0]), CHAIN[1]), quad], mc._cam(), g.sky_color)


@functools.lru_cache(maxsize=None)
def camera_rays(passes, seed=SEED):
    """The oracle's camera rays of mc._cam() over the NX x NY frame: (npx * passes, 7) with time 0 (the test
    scenes hold nothing that moves) and each ray's gradient-sky colour.  The camera ray does not depend on the
    objects, so the oracle's scene is one sphere."""
    import oracle
    o = oracle.build_scene(g.make_scene([g.make_sphere((0.0, 0.0, 0.0), 1.0, _lam(0.5, 0.5, 0.5))], mc._cam(), g.sky_color))
    npx = NX * NY
    rays = np.zeros((npx * passes, 7))
    sky = np.zeros((npx * passes, 3))
    for j in range(npx):
        y, x = divmod(j, NX)
        for smp in range(passes):
            row = o.trace_sample(NX, NY, x, y, seed, smp, cap=1)[0]
            rays[j * passes + smp, 0:6] = row[0:6]
            sky[j * passes + smp] = fc.sky_gradient(row[3:6])
    rays.setflags(write=False)
    sky.setflags(write=False)
    return rays, sky


def mesh_features(scene, passes, smooth=True, seed=SEED):
    """The expected feature buffer (npx, 8) of a scene of meshes only, built as test_gpu_triangles._mesh_features
    builds it: the oracle's camera rays, mesh.hit per leaf in list order, then the leaf's normal — with
    smooth=True mesh.shading_normal where the mesh carries normals, else mesh.normal — the flip, and
    out_of_instance.  Also returns the per-sample rays, t, hit flags and the list position of the leaf hit (-1)."""
    rays, sky = camera_rays(passes, seed)
    n = len(rays)
    t = np.full(n, mesh.TMAX)
    alb, nrm = sky.copy(), np.zeros((n, 3))
    hit = np.zeros(n)
    which = np.full(n, -1)
    for lf in mc.leaves_of(scene):
        local = mesh.into_instance(rays, lf.ops)
        tt, idx = mesh.hit(lf.tris, local)
        take = (idx >= 0) & (tt < t)
        t = np.where(take, tt, t)
        normals = np.zeros((n, 3))
        normals[take] = mesh.normal(lf.tris)[idx[take]]
        if smooth and lf.obj.normals is not None:
            pt = local[:, 0:3] + local[:, 3:6] * tt[:, None]
            vs, fs = lf.obj.args[0], lf.obj.args[1]
            normals[take] = shading_normals_at(vs, fs, lf.obj.normals, pt[take], idx[take])
        if lf.flip:
            normals = normals * -1.0
        nrm[take] = mesh.out_of_instance(normals[take], lf.ops)
        if lf.material.args[0].kind == "constant":                 # (another texture: the caller compares the albedo itself)
            alb[take] = np.array(lf.material.args[0].args[0])
        hit[take] = 1.0
        which[take] = lf.pos
    npx = NX * NY
    per = np.concatenate([alb, nrm, np.where(hit > 0, t, 0.0)[:, None], hit[:, None]], axis=1).reshape(npx, passes, 8)
    feat = np.zeros((npx, 8))
    for smp in range(passes):
        feat = feat + per[:, smp]
    return feat, rays, np.where(hit > 0, t, 0.0), hit, which


# ------------------------------------------------------------------ one scatter step
def _unit_sphere_point(seed, pix, smp, ctr):
    """util.scm:9-15 on the path's stream from draw ctr: (point, the counter after it)."""
    import oracle
    while True:
        a, b, c = oracle.stream(seed, pix, smp, ctr, 3)
        ctr += 3
        p = v.diff(v.scale(v.vec3(a, b, c), 2.0), v.vec3(1.0, 1.0, 1.0))
        if v.dot(p, p) < 1.0:
            return p, ctr


def scatter(pt, nrm, ray, material, seed, pix, smp, ctr, depth=1):
    """One metal (material.scm:45-57) or dielectric (:76-101) step at hit point pt with normal nrm of the path
    whose ray is ray (>= 6 numbers: origin, direction), on the stream of (seed, pix, smp) from draw ctr.
    Returns (survives, origin, direction, attenuation, the counter after the step); an absorbed path (a metal
    reflection below the normal's plane, or the depth cap) has survives False and zeros."""
    import oracle
    d = tuple(float(x) for x in ray[3:6])
    n = tuple(float(x) for x in nrm)
    o = tuple(float(x) for x in pt)
    ctr = int(ctr)
    zero = (0.0, 0.0, 0.0)
    if material.kind == "metal":
        tex, fuzz = material.args
        if tex.kind != "constant":
            raise ValueError("scatter: a constant albedo only")
        reflected = oracle.reflect(v.unit(d), n)
        p, ctr = _unit_sphere_point(seed, pix, smp, ctr)
        direction = v.sum(reflected, v.scale(p, float(fuzz)))
        if depth < KMAX and v.dot(direction, n) > 0:
            return True, o, direction, tuple(float(x) for x in tex.args[0]), ctr
        return False, zero, zero, zero, ctr
    if material.kind == "dielectric":
        ref_idx = float(material.args[0])
        reflected = oracle.reflect(d, n)
        dd = v.dot(d, n)
        outward = v.scale(n, -1.0) if dd > 0 else n
        ni = ref_idx if dd > 0 else 1.0 / ref_idx
        cosine = (dd * ref_idx) / v.length(d) if dd > 0 else (-dd) / v.length(d)
        refracted = oracle.refract(d, outward, ni)
        prob = oracle.schlick(cosine, ref_idx) if refracted is not None else 1.0
        r = oracle.stream(seed, pix, smp, ctr, 1)[0]
        ctr += 1
        direction = reflected if r < prob else refracted
        if depth < KMAX:
            return True, o, direction, (1.0, 1.0, 1.0), ctr
        return False, zero, zero, zero, ctr
    raise ValueError("scatter: metal or dielectric, not %s" % material.kind)


# ------------------------------------------------------- the scatter probe's triangle
TRI = np.array([[-1.0, 0.0, -0.5], [1.25, 0.25, -0.25], [0.0, 0.5, 1.5]])          # one oblique triangle, facing +y
TRI_NORMALS = np.array([[-0.3, 1.0, -0.2], [0.4, 0.9, 0.1], [0.05, 0.8, 0.6]])    # three distinct, none unit


def triangle_scene(material):
    return g.make_scene([g.make_mesh(TRI, np.array([[0, 1, 2]], dtype=np.int32), material, normals=TRI_NORMALS)],
                        make_camera((0, 6, 3), (0, 0, 0), (0, 1, 0), 40, 1.0, 0, 1, 0, 1), g.sky_color)


@functools.lru_cache(maxsize=None)
def triangle_records(n_each=300, seed=7):
    """3 * n_each rays (m, 7) aimed at the triangle's interior, its edges and its vertices, from seeded
    origins on both sides (most above: the side the normals name)."""
    rng = np.random.RandomState(seed)
    b = rng.dirichlet((1.0, 1.0, 1.0), n_each)
    inner = b @ TRI
    e = rng.randint(0, 3, n_each)
    f = rng.uniform(0.0, 1.0, (n_each, 1))
    edge = TRI[e] + (TRI[(e + 1) % 3] - TRI[e]) * f
    vert = TRI[rng.randint(0, 3, n_each)]
    tgt = np.concatenate([inner, edge, vert])
    side = np.where(rng.uniform(size=(len(tgt), 1)) < 0.8, 1.0, -1.0)
    o = tgt + np.concatenate([rng.uniform(-3, 3, (len(tgt), 1)), side * rng.uniform(0.5, 4.0, (len(tgt), 1)),
                              rng.uniform(-3, 3, (len(tgt), 1))], axis=1)
    rays = np.concatenate([o, (tgt - o) * rng.uniform(0.3, 2.0, (len(tgt), 1)), np.zeros((len(tgt), 1))], axis=1)
    rays.setflags(write=False)
    return rays


def throughputs(n):
    return np.random.default_rng([SEED, 11, n]).uniform(0.05, 1.5, size=(n, 3))
