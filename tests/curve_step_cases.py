"""Path states for one step of the persistent curve extend (rt_step_rays on curve-kernel scenes against the
oracle's orc_step), and for the curve and Klein hit records of the group path (no GPU).

k_extend_curves is reached by whole frames only in the other tests, whose rays are camera rays and random
scatters.  Here the records are built from the scenes' own control points, so that the ray meets the curve the
way its class names (hit_ray_cases.py does the same for spheres and rects); tests/test_curve_step_host.py shows,
with the oracle alone, that each class does hit curves.

Scenes (all Cornell-style rooms, open towards -z):
  curves_small   hit_ray_cases' scene: 4096 polyline curves of width 3 in a BVH
  curve_mix      walls, 600 polyline curves, 40 spheres and moving spheres of three materials, a light
  curve_mix_flat the same with 20 000 flat curves (extent ~0.5, width 6: converge's depth estimate is negative, so
                 the root is a leaf and the kernel pools them into stage B)
  dup            300 random curves of width 8, every second and every third one repeated exactly with another
                 material: a tie in z goes to the later curve of the list
  cornell_bezier one curve, below the tree's minimum: a brute-force group (k_extend<kFeatCurves>, group path)
  bezier_inst    that curve under translate(rotate_y(...)): the curve normal d * -1 formed on the local ray
  klein, cornell_klein   the Kleinian limit set: klein_normal

Classes (N records each; a record is a ray with its time and, for `leave`, its draw counter):
  vertical  directions exactly (0, +-1, 0) and (+-0.0, +-2^+-40, +-0.0) through curve points: the ray-space
            transform's dx = dz = 0 branch
  ends      rays through bezier_point(cp, u) + (width / 2) (1 +- 2^-k) w, k = 20, 30, 40, 52, w perpendicular to the
            ray and the curve, u in {0, 1, 2^-k, 1 - 2^-k, 1/2, 1/4, 3/4}: the parameter's ends and the
            subdivision's first split points, either side of the ribbon's edge
  along     rays along an end tangent (P1 - P0, P3 - P2), from outside the end and from the end point itself: the
            curve projects onto (nearly) a point of ray space
  leave     the oracle's own survivors of the tangent / ends / inside records that hit a curve: origin on the
            ribbon, the scattered direction, the counter as it stands; and those origins with the incoming
            direction reversed.  t lies next to t-min
  flat      rays through the flat curves of curve_mix_flat
  dup       rays onto the repeated curves of dup
  moving    depth-0 records with times at the shutter's ends and middle, aimed at a moving sphere where it is at
            that time along a line through a curve point: the curve in front of the sphere or behind it

No record has a non-finite component or a zero direction, and every curve is one a render of these scenes
walks: the curve loops are bounded by the scene (k_extend_curves' ray_cap) and by the curve's depth estimate,
which depends on the curve and the ray's direction up to rotation, not on the ray's length or origin.
"""
import numpy as np

import hit_ray_cases as hc
import scatter_cases as sc
from rtamd import scene as g
from rtamd import scenes
from rtamd import vec as v
from rtamd.rng import HostStream

N = hc.N
SEED = 0x5EED0501
NX, NY = 40, 40
NEW_CURVE_CLASSES = ("vertical", "ends", "along", "leave", "flat", "dup", "moving")
_HC = hc._CURVE_CLASSES


# ------------------------------------------------------------------ scenes
def curve_mix_scene(nx, ny, flat_curves):
    """Curves, spheres and moving spheres in one world BVH between rect groups (the scene of
    test_gpu_parity.test_curve_kernels_bitwise).  flat_curves adds 20 000 short, nearly straight curves whose
    subdivision depth ceil(log4(...)) is negative (bezier.scm:180-193: the root is a leaf)."""
    rr = HostStream(0x5EED0103)
    red = g.make_lambertian(g.constant_texture(v.vec3(0.65, 0.05, 0.05)))
    white = g.make_lambertian(g.constant_texture(v.vec3(0.73, 0.73, 0.73)))
    metal = g.make_metal(g.constant_texture(v.vec3(0.8, 0.8, 0.7)), 0.1)
    glass = g.make_dielectric(1.5)
    light = g.make_diffuse_light(g.constant_texture(v.vec3(4, 4, 4)))
    objs = [g.flip_normals(g.make_yz_rect(0, 555, 0, 555, 555, white)),
            g.make_xz_rect(0, 555, 0, 555, 0, white)]
    objs.append(g.bezier_array(scenes.random_polyline_curves(600), 3.0, red))
    if flat_curves:                  # 20000 tiny curves through the volume, extent ~0.5: half bent
        rs = np.random.default_rng(0x5EED0104)   # by ~1e-3 (maxd -2..-4 at width 6), half straight
        base = rs.uniform(20.0, 535.0, size=(20000, 1, 3))      # (l0 = rounding only, maxd ~ -20)
        t = np.linspace(0.0, 0.5, 4).reshape(1, 4, 1) * rs.normal(size=(20000, 1, 3))
        bend = 1e-3 * rs.normal(size=(20000, 4, 3))
        bend[:10000] = 0.0
        objs.append(g.bezier_array((base + t + bend).reshape(20000, 12), 6.0, white))
    for i in range(40):
        c = v.vec3(60 + rr() * 430, 40 + rr() * 400, 60 + rr() * 430)
        m = (white, metal, glass)[i % 3]
        if i % 4 == 0:
            objs.append(g.make_moving_sphere(c, v.vec3(c[0], c[1] + 20, c[2]), 0.0, 1.0, 15 + 10 * rr(), m))
        else:
            objs.append(g.make_sphere(c, 10 + 15 * rr(), m))
    objs += [g.flip_normals(g.make_xz_rect(213, 343, 227, 332, 554, light)),
             g.make_yz_rect(0, 555, 0, 555, 0, red),
             g.flip_normals(g.make_xy_rect(0, 555, 0, 555, 555, white))]
    return g.make_scene(objs, scenes.cornell_camera_for(nx, ny), g.sky_color)


#: curve_mix's material ids in emit order (white, red, metal, glass, light) and its curve counts
MIX_WHITE, MIX_RED = 0, 1
MIX_POLY, MIX_FLAT = 600, 20000
#: dup's material ids: the floor's, then the three copies'
DUP_FLOOR, DUP_FIRST, DUP_SECOND, DUP_THIRD = 0, 1, 2, 3


def dup_scene(nx, ny):
    """test_gpu_curves.test_duplicate_curves_tie_to_the_later_curve's curves (the floor with a material of its own,
    so that a material names the copy that was hit)."""
    rs = np.random.default_rng(0x5EED0106)
    mats = [g.make_lambertian(g.constant_texture(v.vec3(0.2 + 0.2 * k, 0.5, 0.3))) for k in range(4)]
    cps = rs.uniform(100.0, 450.0, size=(300, 12))
    objs = [g.make_xz_rect(0, 555, 0, 555, 0, mats[0]),
            g.make_bvh_node([g.bezier_array(cps, 8.0, mats[1]), g.bezier_array(cps[::2].copy(), 8.0, mats[2]),
                             g.bezier_array(cps[::3].copy(), 8.0, mats[3])], 0, 0)]
    return g.make_scene(objs, scenes.cornell_camera_for(nx, ny), g.sky_color)


INST_ANGLE, INST_OFFSET = 25.0, (40.0, 30.0, -20.0)
#: bezier_inst's material ids (green, red wall, light, white, the curve's own)
INST_CURVE_MAT = 4
_BEZ = (v.vec3(130, 0, 65), v.vec3(150, 0, 190), v.vec3(130, 0, 190), v.vec3(265, 0, 295))


def bezier_inst_scene(nx, ny):
    """cornell_bezier with its curve under translate(rotate_y(curve, 25), (40, 30, -20)) and a material of its own."""
    red = g.make_lambertian(g.constant_texture(v.vec3(0.65, 0.05, 0.05)))
    white = g.make_lambertian(g.constant_texture(v.vec3(0.73, 0.73, 0.73)))
    green = g.make_lambertian(g.constant_texture(v.vec3(0.12, 0.45, 0.15)))
    light = g.make_diffuse_light(g.constant_texture(v.vec3(3, 3, 3)))
    blue = g.make_lambertian(g.constant_texture(v.vec3(0.1, 0.2, 0.7)))
    curve = g.make_bezier(_BEZ[0], _BEZ[1], _BEZ[2], _BEZ[3], 10, blue)
    objs = [
        g.flip_normals(g.make_yz_rect(0, 555, 0, 555, 555, green)),
        g.make_yz_rect(0, 555, 0, 555, 0, red),
        g.flip_normals(g.make_xz_rect(213, 343, 227, 332, 554, light)),
        g.flip_normals(g.make_xz_rect(0, 555, 0, 555, 555, white)),
        g.make_xz_rect(0, 555, 0, 555, 0, white),
        g.flip_normals(g.make_xy_rect(0, 555, 0, 555, 555, white)),
        g.translate(g.rotate_y(curve, INST_ANGLE), v.vec3(*INST_OFFSET)),
    ]
    return g.make_scene(objs, scenes.cornell_camera_for(nx, ny), g.sky_color)


def _inst_world_cps():
    """bezier_inst's control points in world coordinates (rotate-y, geometry.scm:497-560: x' = cos x + sin z,
    z' = -sin x + cos z; then the offset).  The host test shows that rays aimed at them hit the curve."""
    a = np.radians(INST_ANGLE)
    c, s = np.cos(a), np.sin(a)
    out = []
    for p in _BEZ:
        out += [c * p[0] + s * p[2] + INST_OFFSET[0], p[1] + INST_OFFSET[1], -s * p[0] + c * p[2] + INST_OFFSET[2]]
    return np.array(out).reshape(1, 12)


#: scene -> (constructor(nx, ny), hit_ray_cases classes taken as they are, new classes)
CASES = {
    "curves_small": (scenes.cornell_curves_small, _HC, ("vertical", "ends", "along", "leave")),
    "curve_mix": (lambda nx, ny: curve_mix_scene(nx, ny, False), _HC, ("vertical", "ends", "along", "leave", "moving")),
    "curve_mix_flat": (lambda nx, ny: curve_mix_scene(nx, ny, True), (), ("flat", "leave")),
    "dup": (dup_scene, (), ("dup", "vertical", "ends")),
}
#: the group-path scenes (no curve kernel: k_extend<F>): scene -> (constructor, classes)
GROUP_CASES = {
    "cornell_bezier": (scenes.cornell_bezier, ("vertical", "ends", "leave")),
    "bezier_inst": (bezier_inst_scene, ("vertical", "ends", "leave")),
    "klein": (scenes.klein_scene, ("klein", "klein_leave")),
    "cornell_klein": (scenes.cornell_klein, ("klein", "klein_leave")),
}
#: material id of the limit set (klein: the ground's, then the set's; cornell_klein: green, red, light, white, blue)
KLEIN_MAT = {"klein": 1, "cornell_klein": 4}


# ------------------------------------------------------------------ helpers
def bezier_tangent(cp, u):
    a, b, c, d = cp[0:3], cp[3:6], cp[6:9], cp[9:12]
    w = 1.0 - u
    return 3 * w * w * (b - a) + 6 * w * u * (c - b) + 3 * u * u * (d - c)


def _aim_curves(P):
    """The curves rays are aimed at: every curve, by default."""
    return np.arange(len(P.cps))


class Recs:
    """A class's records: rays (n, 7) and the draw counters (n,) they start from."""

    def __init__(self, rays, ctr=None):
        self.rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 7)
        self.ctr = np.zeros(len(self.rays), dtype=np.uint32) if ctr is None else np.asarray(ctr, dtype=np.uint32)
        assert np.isfinite(self.rays).all() and (np.abs(self.rays[:, 3:6]).max(axis=1) > 0).all()

    def __len__(self):
        return len(self.rays)


# ------------------------------------------------------------------ classes
def rays_vertical(P, rng, n=N, pool=None):
    R = hc.Rays()
    pool = _aim_curves(P) if pool is None else pool
    for k in range(n):
        j = int(rng.choice(pool))
        p = hc.bezier_point(P.cps[j], rng.uniform())
        sy = 1.0 if (k % 2) == 0 else -1.0
        if (k // 2) % 3 == 0:
            d = np.array([0.0, sy, 0.0])
        else:
            z = (0.0, -0.0)[(k // 6) % 2]
            d = np.array([z, sy * 2.0 ** (40 if (k // 2) % 3 == 1 else -40), -z if (k // 12) % 2 else z])
        if (k // 4) % 3 == 2:                       # beside the curve: another curve, a wall, the floor or the sky
            p = p + np.array([1.0, 0.0, -1.0]) * P.width[j] * rng.uniform(0.8, 12.0)
        dist = rng.uniform(2.0, 60.0) * max(1.0, P.width[j])
        R.add(p - (dist / abs(d[1])) * d, d, 0.0, "v")
    return R.done()[0]


_END_K = (20, 30, 40, 52)


def _from_above(d, w):
    """d heading down and the offset w on the upper side: the ray meets the curve before a floor the curve lies in"""
    d = np.where(np.arange(3) == 1, -np.abs(d), d)
    return d, (w if w[1] >= 0 else -w)


def rays_ends(P, rng, n=N, pool=None, above=False):
    R = hc.Rays()
    pool = _aim_curves(P) if pool is None else pool
    for k in range(n):
        e = _END_K[k % 4]
        u = (0.0, 1.0, 2.0 ** -e, 1.0 - 2.0 ** -e, 0.5, 0.25, 0.75)[(k // 4) % 7]
        side = 1.0 - 2.0 ** -e if (k // 28) % 2 == 0 else 1.0 + 2.0 ** -e
        j = int(rng.choice(pool))
        cp = P.cps[j]
        c, tan = hc.bezier_point(cp, u), bezier_tangent(cp, u)
        d = rng.normal(size=3)
        if above:
            d[1] = -abs(d[1])
        w = np.cross(d, tan)
        w = w / np.linalg.norm(w) if np.linalg.norm(w) > 1e-6 * np.linalg.norm(d) * max(np.linalg.norm(tan), 1e-300) \
            else hc.perp(d, rng)
        if above:
            d, w = _from_above(d, w)
        d = hc.unit(d) * (1.0, 0.25, 7.0)[k % 3]
        p = c + (P.width[j] / 2 * side) * w
        far = rng.uniform(1.5, 12.0) * P.width[j]
        R.add(p - (far / np.linalg.norm(d)) * d, d, 0.0, "in" if side < 1 else "out")
    return R.done()[0]


def rays_along(P, rng, n=N, pool=None):
    R = hc.Rays()
    pool = _aim_curves(P) if pool is None else pool
    for k in range(n):
        j = int(rng.choice(pool))
        cp = P.cps[j]
        if (k // 2) % 2 == 0:
            end, tan = cp[0:3], cp[3:6] - cp[0:3]           # into the curve from P0, along P1 - P0
        else:
            end, tan = cp[9:12], cp[6:9] - cp[9:12]         # into the curve from P3, along P2 - P3
        if not np.linalg.norm(tan) > 0:
            tan = cp[9:12] - cp[0:3]
        d = tan * (1.0, 0.25, 7.0)[k % 3] if (k // 4) % 2 == 0 else hc.unit(tan)
        o = end.copy()
        if k % 2 == 0:                                      # from outside the end
            o = end - hc.unit(tan) * rng.uniform(0.5, 8.0) * P.width[j]
        if (k // 8) % 4 == 3:                               # beside the ribbon, parallel to the tangent
            o = o + hc.perp(tan, rng) * P.width[j] * rng.uniform(0.6, 2.5)
        if (k // 8) % 8 == 5:                               # away from the curve, out of its end
            d = -d
        R.add(o, d, 0.0, "along")
    return R.done()[0]


def rays_on_curves(P, rng, pool, n=N, miss_every=4, above=False, escape=False):
    """Rays of random directions through points of the pool's ribbons (within 0.8 of the half width), one in
    miss_every beside the ribbon; escape (a cloud so dense that a ray beside one curve meets another): every
    second of those starts in front of the cloud and heads out of the room's open side."""
    R = hc.Rays()
    for k in range(n):
        j = int(rng.choice(pool))
        cp = P.cps[j]
        u = rng.uniform()
        c, tan = hc.bezier_point(cp, u), bezier_tangent(cp, u)
        d = rng.normal(size=3) * (1.0, 0.25, 7.0)[k % 3]
        if above:
            d[1] = -abs(d[1])
        w = np.cross(d, tan)
        w = w / np.linalg.norm(w) if np.linalg.norm(w) > 0 else hc.perp(d, rng)
        if above:
            d, w = _from_above(d, w)
        off = rng.uniform(-0.8, 0.8) if k % miss_every != miss_every - 1 else rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 24.0)
        p = c + (P.width[j] / 2 * off) * w
        if escape and k % (2 * miss_every) == miss_every - 1:
            d = hc.escape_dir(P, rng) * np.linalg.norm(d)
            p[2] = P.cps[:, 2::3].min() - 2.0 * P.width[j]
            R.add(p, d, 0.0, "escape")
            continue
        R.add(p - (rng.uniform(1.0, 8.0) * P.width[j] / np.linalg.norm(d)) * d, d, 0.0, "on")
    return R.done()[0]


def rays_moving(P, rng, n=N):
    R = hc.Rays()
    t0, t1 = P.shutter
    mov = [i for i in P.small if P.moving[i]]
    for k in range(n):
        tm = (t0, t1, 0.5 * (t0 + t1))[k % 3]
        i = int(rng.choice(mov))
        c, r = P.centre(i, tm), P.r[i]
        # a point of the sphere's disc as seen along d: inside it, or just outside it on the y side it moves along
        q = hc.bezier_point(P.cps[int(rng.integers(len(P.cps)))], rng.uniform())
        aim = c + hc.unit(rng.normal(size=3)) * r * (rng.uniform(0.0, 0.9) if (k // 3) % 3 != 2 else rng.uniform(1.02, 1.6))
        d = hc.unit(aim - q)
        if (k // 9) % 2 == 0:                               # the curve point in front of the sphere
            o = q - d * rng.uniform(3.0, 30.0)
        else:                                               # the sphere in front, the curve point behind it
            o = aim + d * (2.0 * r + rng.uniform(1.0, 20.0))
            d = -d
        R.add(o, d * (1.0, 0.5, 3.0)[(k // 18) % 3], tm, "moving")
    return R.done()[0]


def leave_records(osc, sources, n=N):
    """The oracle's survivors of `sources` (Recs) that hit a curve: half as they scatter (origin on the ribbon,
    the scattered direction, the counter after the scatter), half with the incoming direction reversed."""
    import oracle
    rays, ctrs = [], []
    for src in sources:
        with np.errstate(all="ignore"):
            rows, ctr = osc.step(src.rays, 1, sc.SEED, sc.SMP, ctr_in=src.ctr)
        on = curve_hit(rows, src.rays) & (rows[:, oracle.STEP_KIND] == 1)
        for k in np.flatnonzero(on):
            o, d = rows[k, oracle.STEP_O], rows[k, oracle.STEP_D]
            rays.append(np.concatenate([o, d, [0.0]]))
            ctrs.append(ctr[k])
            rays.append(np.concatenate([o, -src.rays[k, 3:6], [0.0]]))
            ctrs.append(ctr[k])
    rays, ctrs = np.array(rays).reshape(-1, 7), np.array(ctrs, dtype=np.uint32)
    pick = np.random.default_rng([SEED, 99]).permutation(len(rays))[:n]
    pick.sort()
    return Recs(rays[pick], ctrs[pick])


def curve_hit(rows, rays):
    """orc_step rows whose closest hit is a curve outside every instance: the record's normal is -d bit for bit
    (bezier.scm:204; a sphere's, rect's or Klein normal equal to -d in all three doubles does not occur)."""
    import oracle
    return (rows[:, oracle.STEP_HIT] == 1) & sc.same_bits(rows[:, oracle.STEP_N], -rays[:, 3:6]).all(axis=1)


def curve_hits(name, rows, rays):
    """curve_hit for any scene of this module: under bezier_inst's chain the curve's hits are its material's."""
    import oracle
    if name == "bezier_inst":
        return (rows[:, oracle.STEP_HIT] == 1) & (rows[:, oracle.STEP_MAT] == INST_CURVE_MAT)
    return curve_hit(rows, rays)


# ------------------------------------------------------------------ the case sets
_scene_cache, _osc_cache, _rec_cache = {}, {}, {}


def scene(name):
    if name not in _scene_cache:
        make = (CASES.get(name) or GROUP_CASES[name])[0]
        _scene_cache[name] = make(NX, NY)
    return _scene_cache[name]


def oracle_scene(oracle_mod, name):
    if name not in _osc_cache:
        _osc_cache[name] = oracle_mod.build_scene(scene(name))
    return _osc_cache[name]


def prims(name):
    P = hc.Prims(scene(name))
    if name == "bezier_inst":
        P.cps = _inst_world_cps()
    return P


def _pool(name, P, cls):
    if cls == "flat":
        return np.arange(MIX_POLY, MIX_POLY + MIX_FLAT)
    if name == "dup":                                       # curves with a copy (every second and third one)
        return np.array([j for j in range(300) if j % 2 == 0 or j % 3 == 0])
    if name == "curve_mix_flat":
        return np.arange(MIX_POLY)
    return _aim_curves(P)


def records(oracle_mod, name):
    """{class: Recs} of a scene, seeded per (scene, class) and cached.  The hit_ray_cases classes come first, as
    hit_ray_cases builds them for the scene's primitives; `leave` is built last, from the oracle's steps."""
    if name in _rec_cache:
        return _rec_cache[name]
    if name in KLEIN_MAT:
        _rec_cache[name] = _klein_records(oracle_mod, name)
        return _rec_cache[name]
    old, new = (CASES[name][1], CASES[name][2]) if name in CASES else ((), GROUP_CASES[name][1])
    P = prims(name)
    out = {}
    with np.errstate(all="ignore"):
        for ci, cls in enumerate(hc.CLASSES):
            if cls in old:
                out[cls] = Recs(hc._BUILDERS[cls](P, np.random.default_rng([hc.SEED, ci]))[0])
        for ci, cls in enumerate(NEW_CURVE_CLASSES):
            if cls not in new or cls == "leave":
                continue
            rng = np.random.default_rng([SEED, ci, len(name)])
            pool = _pool(name, P, cls)
            if cls == "vertical":
                out[cls] = Recs(rays_vertical(P, rng, pool=pool))
            elif cls == "ends":
                out[cls] = Recs(rays_ends(P, rng, pool=pool, above=name in GROUP_CASES))
            elif cls == "along":
                out[cls] = Recs(rays_along(P, rng, pool=pool))
            elif cls in ("flat", "dup"):
                out[cls] = Recs(rays_on_curves(P, rng, pool, escape=cls == "dup"))
            elif cls == "moving":
                out[cls] = Recs(rays_moving(P, rng))
        if "leave" in new:
            osc = oracle_scene(oracle_mod, name)
            if name in GROUP_CASES:
                rng = np.random.default_rng([SEED, 50, len(name)])
                src = [out["ends"], Recs(rays_on_curves(P, rng, _aim_curves(P), above=True))]
                out["leave"] = leave_records(osc, src) if name != "bezier_inst" else _inst_leave(osc, src)
            else:
                rng = np.random.default_rng([SEED, 51, len(name)])
                pool = _pool(name, P, "flat" if name == "curve_mix_flat" else "leave")
                src = [Recs(hc.rays_tangent(_curves_only(P), rng)[0]), Recs(rays_ends(P, rng, pool=pool)),
                       Recs(rays_on_curves(P, rng, pool)), Recs(hc.rays_inside(_curves_only(P), rng)[0])]
                out["leave"] = leave_records(osc, src)
    _rec_cache[name] = out
    return out


def _curves_only(P):
    """P with its spheres hidden, so that hit_ray_cases' builders take their curve branches."""
    import copy
    Q = copy.copy(P)
    Q.small = np.array([], dtype=int)
    Q.r = np.array([])
    return Q


def _inst_leave(osc, sources, n=N):
    """leave_records for the curve under an instance, whose world normal is not -d bit for bit: the curve's
    hits are those of its material."""
    import oracle
    rays, ctrs = [], []
    for src in sources:
        with np.errstate(all="ignore"):
            rows, ctr = osc.step(src.rays, 1, sc.SEED, sc.SMP, ctr_in=src.ctr)
        on = (rows[:, oracle.STEP_HIT] == 1) & (rows[:, oracle.STEP_MAT] == INST_CURVE_MAT) & (rows[:, oracle.STEP_KIND] == 1)
        for k in np.flatnonzero(on):
            for d in (rows[k, oracle.STEP_D], -src.rays[k, 3:6]):
                rays.append(np.concatenate([rows[k, oracle.STEP_O], d, [0.0]]))
                ctrs.append(ctr[k])
    rays, ctrs = np.array(rays).reshape(-1, 7), np.array(ctrs, dtype=np.uint32)
    pick = np.sort(np.random.default_rng([SEED, 98]).permutation(len(rays))[:n])
    return Recs(rays[pick], ctrs[pick])


def _klein_records(oracle_mod, name, n=N):
    """klein: camera-like rays (the camera's origin, through film points; raw and unit directions), three in four
    of them hitting the limit set by the oracle; klein_leave: the oracle's survivors of those hits (origin next to
    the surface just left, the scattered direction, the counter as it stands)."""
    import oracle
    s = scene(name)
    osc = oracle_scene(oracle_mod, name)
    cam = np.array(s.camera.slots())
    rng = np.random.default_rng([SEED, 60, len(name)])
    # klein-scene's camera sees little of its set (about one film point in a hundred): there the rays leave the
    # camera's origin towards points around the set's centre, and those the oracle's closest hit puts on the set
    # are kept, with a quarter of others
    centre = next(np.asarray(o.args[0], dtype=float) for o in s.obj_list if o.kind == "klein")
    want_on, want_off = 3 * n // 4, n - 3 * n // 4
    on_rays, off_rays = [], []
    for tries in range(400 * n):
        if len(on_rays) >= want_on and len(off_rays) >= want_off:
            break
        if name == "klein":
            d = centre + rng.normal(size=3) * 2.0 - cam[9:12]
        else:
            d = cam[0:3] + rng.uniform() * cam[3:6] + rng.uniform() * cam[6:9] - cam[9:12]
        if tries % 4 == 3:                                  # (the set's march depends on |d|: few unit rays reach it)
            d = d / np.linalg.norm(d)
        with np.errstate(all="ignore"):
            h = osc.hit_world(cam[9:12], d, 0.0)
        hit_set = h is not None and int(h[7]) == KLEIN_MAT[name]
        if hit_set and len(on_rays) < want_on:
            on_rays.append(np.concatenate([cam[9:12], d, [0.0]]))
        elif not hit_set and len(off_rays) < want_off:
            off_rays.append(np.concatenate([cam[9:12], d, [0.0]]))
    rays = np.array(on_rays + off_rays).reshape(-1, 7)
    rays = rays[np.random.default_rng([SEED, 61]).permutation(len(rays))]
    with np.errstate(all="ignore"):
        rows, ctr = osc.step(rays, 1, sc.SEED, sc.SMP)
    on = (rows[:, oracle.STEP_HIT] == 1) & (rows[:, oracle.STEP_MAT] == KLEIN_MAT[name])
    take = np.arange(len(rays))
    sv = np.flatnonzero(on & (rows[:, oracle.STEP_KIND] == 1))[:n]
    left = np.concatenate([rows[sv][:, oracle.STEP_O], rows[sv][:, oracle.STEP_D], np.zeros((len(sv), 1))], axis=1)
    return {"klein": Recs(rays[take]), "klein_leave": Recs(left, ctr[sv])}


def mixed(oracle_mod, name="curve_mix", n=None):
    """The scene's time-0 classes one after the other, tiled to n records: (rays, ctr)."""
    recs = [r for c, r in records(oracle_mod, name).items() if c != "moving"]
    rays, ctr = np.concatenate([r.rays for r in recs]), np.concatenate([r.ctr for r in recs])
    if n is None:
        return rays, ctr
    reps = (n + len(rays) - 1) // len(rays)
    return np.concatenate([rays] * max(1, reps))[:n], np.concatenate([ctr] * max(1, reps))[:n]


def quick_hits(oracle_mod, name="curve_mix", n=None):
    """Records that all reach a hit within a few steps (the `leave` and `inside` classes): many park at once in
    the fused extend's ring."""
    r = records(oracle_mod, name)
    rays = np.concatenate([r["leave"].rays, r["inside"].rays])
    ctr = np.concatenate([r["leave"].ctr, r["inside"].ctr])
    if n is None:
        return rays, ctr
    reps = (n + len(rays) - 1) // len(rays)
    return np.concatenate([rays] * reps)[:n], np.concatenate([ctr] * reps)[:n]
