"""Path states for one scatter step (rt_step_rays against the oracle's orc_step): scenes plus named record classes.

Hit points are exact by construction wherever a class depends on them: axis-parallel rays onto rects with t a
small power of two, so o + d * t has no rounding and the texture, the onb and the light densities see the
coordinates the class names.  A record is a ray (origin, direction, time); the tests run the same records at
several depths, draw counters and throughputs.

The panel scene: a row of xz rects at y = 1 (off y = 0, where sin(0) would make every checker point even),
panel i covering z in [4 i - 1, 4 i + 1] and x in [-2^21, 2^21], one material each, hit from above or below
by vertical rays; behind them, at y = 10 and z = -20, a row of spheres, an instanced box and the two other rect
kinds, hit by rays along z and x.  Nothing shadows anything on those rays.
"""
import math

import numpy as np

import hit_ray_cases as hc
from rtamd import perlin as _perlin
from rtamd import scene as g
from rtamd import vec as v
from rtamd.camera import make_camera
from rtamd.scenes import PERLIN_SEED

SEED = 0x5EED0401
SMP = 3
KMAX = 100                       # kMaxDepth (rt_device.h), ORC_MAX_DEPTH
XMAX = float(2 ** 21)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_LIGHT = 0, 1, 2, 3
PI10 = math.pi / 10.0

PANELS = ("checker", "checker_nested", "noise", "marble", "checker_noise", "metal0", "metal_half", "metal1",
          "glass", "glass1", "light", "light_flip", "light_noise", "plain", "plain_flip")


def _c(r, gg, b):
    return g.constant_texture(v.vec3(r, gg, b))


def _cam():
    return make_camera(v.vec3(0, 5, 30), v.vec3(0, 5, 0), v.vec3(0, 1, 0), 40, 1.0, 0, 1, 0, 1)


def panel_z(name):
    return 4.0 * PANELS.index(name)


def panel_scene(noise=True, light=None, image=False, many=False, tri=False):
    """The panel scene.  noise: the noise / marble textures (False: constants in their place, so no Perlin
    tables).  light: None, "single" (rt_set_light_sampling of the light panel) or "twice" (a light list naming
    that panel twice: the mixture's list code with the densities of the single light).  image / many / tri:
    decoys no probe ray can reach (10^7 away): an image-textured sphere, 300 small spheres, a triangle."""
    nz = (lambda s: g.noise_texture(s)) if noise else (lambda s: _c(0.5, 0.5, 0.5))
    mb = (lambda s: g.marble_texture(s)) if noise else (lambda s: _c(0.4, 0.6, 0.5))
    ck = g.checker_texture(_c(0.2, 0.3, 0.1), _c(0.9, 0.9, 0.9))
    mats = {
        "checker": g.make_lambertian(ck),
        "checker_nested": g.make_lambertian(g.checker_texture(g.checker_texture(_c(0.1, 0.2, 0.9), _c(0.9, 0.2, 0.1)),
                                                              _c(0.3, 0.8, 0.3))),
        "noise": g.make_lambertian(nz(4.0)),
        "marble": g.make_lambertian(mb(2.0)),
        "checker_noise": g.make_lambertian(g.checker_texture(nz(1.0), mb(3.0))),
        "metal0": g.make_metal(_c(0.7, 0.6, 0.5), 0.0),
        "metal_half": g.make_metal(ck, 0.5),
        "metal1": g.make_metal(nz(2.0), 1.0),
        "glass": g.make_dielectric(1.5),
        "glass1": g.make_dielectric(1.0),
        "light": g.make_diffuse_light(_c(4, 3, 2)),
        "light_flip": g.make_diffuse_light(ck),
        "light_noise": g.make_diffuse_light(nz(4.0)),
        "plain": g.make_lambertian(_c(0.73, 0.73, 0.73)),
        "plain_flip": g.make_lambertian(_c(0.12, 0.45, 0.15)),
    }
    objs = []
    the_light = None
    for name in PANELS:
        z = panel_z(name)
        r = g.make_xz_rect(-XMAX, XMAX, z - 1.0, z + 1.0, 1.0, mats[name])
        if name == "light":
            # the sampled light: a small one, so its densities are not tiny
            r = g.make_xz_rect(-2.0, 2.0, z - 1.0, z + 1.0, 1.0, mats[name])
            the_light = r
        if name in ("light_flip", "plain_flip"):
            r = g.flip_normals(r)
        objs.append(r)
    # a far marble panel: large |z| in the marble's sine
    objs.append(g.make_xz_rect(-1.0, 1.0, 2.0 ** 20 - 1.0, 2.0 ** 20 + 1.0, 1.0, mats["marble"]))
    # the row behind: spheres of radius 2 (a power of two: the normal's division is exact) at y = 10, z = -20
    objs += [
        g.make_sphere(v.vec3(0, 10, -20), 2.0, mats["noise"]),
        g.make_sphere(v.vec3(8, 10, -20), 2.0, mats["glass"]),
        g.make_sphere(v.vec3(8, 10, -20), -1.75, mats["glass"]),
        g.make_moving_sphere(v.vec3(16, 10, -20), v.vec3(16, 10.5, -20), 0, 1, 2.0, mats["plain"]),
        g.make_sphere(v.vec3(24, 10, -20), 2.0, mats["marble"]),
        g.make_sphere(v.vec3(32, 10, -20), 2.0, mats["metal_half"]),
        g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(2, 2, 2), mats["plain"]), 30), v.vec3(40, 9, -20)),
        g.make_xy_rect(48, 50, 9, 11, -20, mats["checker"]),
        g.flip_normals(g.make_xy_rect(52, 54, 9, 11, -20, mats["checker"])),
        g.make_yz_rect(9, 11, -21, -19, 60, mats["plain"]),
        g.flip_normals(g.make_yz_rect(9, 11, -21, -19, 70, mats["plain"])),
    ]
    far = 1.0e7
    if many:
        objs += [g.make_sphere(v.vec3(far + 3.0 * k, far, far), 1.0, mats["plain"]) for k in range(300)]
    if image:
        tex = g.make_image_texture(bytes(range(48)), 4, 4)
        objs.append(g.make_sphere(v.vec3(far, -far, far), 1.0, g.make_lambertian(tex)))
    if tri:
        objs.append(g.make_triangle(v.vec3(-far, far, far), v.vec3(-far + 1, far, far), v.vec3(-far, far + 1, far),
                                    mats["plain"]))
    kw = {}
    if light == "single":
        kw["light"] = the_light
    elif light == "twice":
        kw["lights"] = [the_light, the_light]
    return g.make_scene(objs, _cam(), g.sky_color, perlin=_perlin.from_seed(PERLIN_SEED) if noise else None, **kw)


def oracle_twin(oracle_mod, noise=True, light=None):
    """The oracle's scene for a panel variant: without the decoys (it knows neither images nor triangles, and
    no ray reaches any of them).  "twice": the single light's scene with the oracle's own list rule over that
    light named twice (OracleScene.set_light_list; rtamd.scene.emit hands light lists to the GPU builder only)."""
    o = oracle_mod.build_scene(panel_scene(noise=noise, light="single" if light else None))
    if light == "twice":
        o.set_light_list([o.light_obj, o.light_obj])
    return o


# ------------------------------------------------------------------ records
class Recs:
    def __init__(self):
        self.r = []

    def add(self, o, d, tm=0.0):
        self.r.append([o[0], o[1], o[2], d[0], d[1], d[2], tm])

    def down(self, x, z, speed=1.0, y=1.0, t=2.0):
        """a vertical ray onto the plane y from above: the hit point is (x, y, z) exactly, at t"""
        self.add((x, y + speed * t, z), (math.copysign(0.0, x), -speed, math.copysign(0.0, z)))

    def up(self, x, z, speed=1.0, y=1.0, t=2.0):
        self.add((x, y - speed * t, z), (math.copysign(0.0, x), speed, math.copysign(0.0, z)))

    def done(self):
        return np.array(self.r, dtype=np.float64).reshape(-1, 7)


def _ulps(x, ks=(-1, 0, 1)):
    out = []
    for k in ks:
        y = x
        for _ in range(abs(k)):
            y = np.nextafter(y, math.inf if k > 0 else -math.inf)
        out.append(float(y))
    return out


def checker_points():
    """x (and, on the first panel, z) coordinates where sin(10 x) is at or next to a zero: fl(k pi / 10) for
    small k and one large k (|10 x| >= 2^20), each with its two neighbours; +-0.0; and plain large values."""
    xs = []
    for k in (1, 2, 3, 7, -1, -5, 4000000, -4000001):
        xs += _ulps(k * PI10)
    xs += [0.0, -0.0, 2.0 ** 17, 2.0 ** 17 + 0.5, -(2.0 ** 20) - 0.25, 0.3, -0.7]
    return xs


def recs_checker():
    R = Recs()
    for name in ("checker", "checker_nested", "metal_half", "light_flip"):
        z0 = panel_z(name)
        for x in checker_points():
            if name == "light_flip":
                R.up(x, z0 + 0.25)
            else:
                R.down(x, z0 + 0.25)
    for z in _ulps(PI10) + _ulps(-PI10) + _ulps(3 * PI10) + [0.0, -0.0]:     # panel 0: z near a zero too
        for x in (0.3, PI10, -0.0):
            R.down(x, z)
    return R.done()


def recs_noise():
    R = Recs()
    below = lambda q: float(np.nextafter(q, -math.inf))
    # scale 4 on "noise" / "light_noise", 2 on "marble" / "metal1", 1 and 3 on "checker_noise"
    for name, sc in (("noise", 4.0), ("marble", 2.0), ("metal1", 2.0), ("light_noise", 4.0), ("checker_noise", 1.0)):
        z0 = panel_z(name)
        for q in (0.0, 1.0, 3.0, -1.0, -2.0, 255.0, 256.0, 257.0, -255.0, -256.0, -257.0, 0.5, -0.5, 100.25):
            for x in (q / sc, below(q / sc)):
                for dz in (0.0, 0.25, -0.5, 0.3):
                    R.down(x, z0 + dz)
    for x in (0.0, 0.5, -0.75):                       # marble with large |z|
        for dz in (0.0, 0.5, -0.3):
            R.down(x, 2.0 ** 20 + dz)
    # the noise and marble spheres, by rays along -z
    for cx in (0.0, 24.0):
        for dx in (0.0, 0.5, -1.0, 1.25, -1.9):
            for dy in (0.0, 0.75, -1.5):
                if dx * dx + dy * dy < 3.9:
                    R.add((cx + dx, 10.0 + dy, 0.0), (0.0, 0.0, -1.0))
    return R.done()


def recs_onb():
    """Normals on both sides of the |n.x| > 0.9 switch: x = +-1.8 (+- a few ulps) on a sphere of radius 2 centred
    at x = 0 gives n.x = fl(0.9) and its neighbours; the axis normals of the three rect kinds and their flips;
    the rotated and translated box; the moving sphere at a time != 0 (depth 0 only: see recs_time)."""
    R = Recs()
    for sx in (1.0, -1.0):
        for x in _ulps(1.8, (-4, -2, -1, 0, 1, 2, 4)) + [1.75, 1.85, 1.0, 0.0]:
            for dy in (0.0, 0.3):
                R.add((sx * x, 10.0 + dy, 0.0), (0.0, 0.0, -1.0))
    for name in ("plain", "plain_flip"):              # xz rect and its flip, from both sides
        R.down(0.5, panel_z(name))
        R.up(0.5, panel_z(name))
    for x in (49.0, 53.0):                            # xy rect and its flip, from both sides
        R.add((x, 10.0, -18.0), (0.0, 0.0, -1.0))
        R.add((x, 10.0, -22.0), (0.0, 0.0, 1.0))
    R.add((62.0, 10.0, -20.0), (-1.0, 0.0, 0.0))      # yz rect and its flip
    R.add((58.0, 10.0, -20.0), (1.0, 0.0, 0.0))
    R.add((68.0, 10.0, -20.0), (1.0, 0.0, 0.0))
    R.add((72.0, 10.0, -20.0), (-1.0, 0.0, 0.0))
    for dx in (0.3, 0.9, 1.6, 2.2):                   # the instance: rotate-y 30 then translate
        for dy in (0.5, 1.5):
            R.add((40.0 + dx, 9.0 + dy, 0.0), (0.0, 0.0, -1.0))
            R.add((40.0 + dx, 20.0, -20.5 + dy), (0.0, -1.0, 0.0))
    return R.done()


def recs_time():
    """The moving sphere at times != 0 (depth 0 only: every scattered ray has time +0.0)."""
    R = Recs()
    for tm in (0.0, 0.25, 0.5, 1.0):
        for dx in (0.0, 0.9, -1.7):
            R.add((16.0 + dx, 10.2, 0.0), (0.0, 0.0, -1.0), tm)
    return R.done()


def recs_metal():
    R = Recs()
    for name in ("metal0", "metal_half", "metal1"):
        z0 = panel_z(name)
        for speed in (0.3, 1.0, 7.0):
            for x in (0.25, -3.5, 17.0):
                R.down(x, z0 + 0.25, speed=speed)
        for k in range(24):                            # grazing: a fuzzed reflection then often points below
            gy = 2.0 ** -(2 + k % 12)
            R.add((0.5 * k - 2.0, 1.0 + 2.0 * gy, z0 - 0.5), (1.0, -gy, 0.0))
        for k in range(8):
            a = 0.2 + 0.17 * k
            R.add((-2.0 * math.sin(a), 1.0 + 2.0 * math.cos(a), z0), (math.sin(a), -math.cos(a), 0.0))
    for dx in (0.0, 1.0, 1.9, 1.99):                   # the metal sphere
        R.add((32.0 + dx, 10.0, 0.0), (0.0, 0.0, -1.0))
    return R.done()


CRIT = math.asin(1.0 / 1.5)


def recs_dielectric():
    """From outside (down onto the panel) and inside (up from below: dot(d, n) > 0): normal incidence, a sweep
    across the critical angle of 1.5 (inside) down to single ulps of the direction, near-tangent, |d| != 1,
    ref_idx 1, the sphere with its negative-radius shell."""
    R = Recs()
    z0, z1 = panel_z("glass"), panel_z("glass1")
    for z in (z0, z1):
        R.down(0.5, z)
        R.up(0.5, z)
        for speed in (0.3, 7.0):
            R.down(0.5, z + 0.5, speed=speed)
            R.up(0.5, z + 0.5, speed=speed)
        for a in (0.1, 0.5, 1.0, 1.4, 1.5, 1.57, 1.5707963):          # oblique to near-tangent, both sides
            for sc in (1.0, 0.3, 7.0):
                s, c = math.sin(a) * sc, math.cos(a) * sc
                R.add((-2.0 * s, 1.0 + 2.0 * c, z), (s, -c, 0.0))
                R.add((-2.0 * s, 1.0 - 2.0 * c, z), (s, c, 0.0))
    return np.concatenate([R.done(), recs_critical(), recs_shell()])


def recs_critical():
    """The sweep: directions (sin a, cos a, 0) from inside the glass panel with a = critical angle + delta, delta
    from 1e-1 down to 1e-16 on both sides, then sin a stepped by 0, 1, 2, 4 and 8 ulps either way at fixed cos a."""
    R = Recs()
    z0 = panel_z("glass")
    for e in range(1, 17):
        for sg in (1.0, -1.0):
            a = CRIT + sg * 10.0 ** -e
            s, c = math.sin(a), math.cos(a)
            R.add((-2.0 * s, 1.0 - 2.0 * c, z0), (s, c, 0.0))
    s0, c0 = math.sin(CRIT), math.cos(CRIT)
    for s in _ulps(s0, (-8, -4, -2, -1, 0, 1, 2, 4, 8)):
        R.add((-2.0 * s, 1.0 - 2.0 * c0, z0), (s, c0, 0.0))
        R.add((-2.0 * s, 1.0 - 2.0 * c0, z0 + 0.5), (s * 3.0, c0 * 3.0, 0.0))
    return R.done()


def recs_shell():
    R = Recs()
    for dx in (0.0, 0.5, 1.5, 1.8, 1.99):
        R.add((8.0 + dx, 10.0, 0.0), (0.0, 0.0, -1.0))            # into the outer sphere
        R.add((8.0 + dx * 0.05, 10.0, -18.1), (0.0, 0.0, 1.0))    # between shell and surface, outward
        R.add((8.0 + dx * 0.05, 10.0, -18.1), (0.0, 0.0, -1.0))   # ... inward, onto the shell
        R.add((8.0 + dx * 0.5, 10.0, -20.0), (0.0, 0.0, 1.0))     # from the centre onto the shell
    return R.done()


def recs_lights():
    R = Recs()
    for name in ("light", "light_flip", "light_noise"):
        z0 = panel_z(name)
        for x in (0.0, 0.5, -1.5, PI10):
            R.down(x, z0 + 0.25)
            R.up(x, z0 + 0.25)
            R.add((x - 1.0, 3.0, z0), (0.5, -1.0, 0.0))
            R.add((x - 1.0, -1.0, z0), (0.5, 1.0, 0.0))
    return R.done()


def recs_mixture():
    """Lambertian points for the light mixture of the panel scene's light (the "light" panel, x in [-2, 2]):
    on the light's own plane beside it (every other panel: a direction to the light lies in the plane, both
    densities are 0 and the path ends), hit from above and from below."""
    R = Recs()
    for name in ("plain", "checker", "noise", "marble"):
        z0 = panel_z(name)
        for x in (0.0, 1.5, -3.0, 40.0):
            for dz in (0.0, 0.5, -0.75):
                R.down(x, z0 + dz)
                R.up(x, z0 + dz)
    for dx in (0.0, 0.5, 1.5):                          # sphere and instance points: the light is below them
        R.add((dx, 10.0, 0.0), (0.0, 0.0, -1.0))
        R.add((16.0 + dx, 10.0, 0.0), (0.0, 0.0, -1.0))
        R.add((40.5 + dx, 10.0, 0.0), (0.0, 0.0, -1.0))
    return R.done()


def recs_miss():
    R = Recs()
    for d in ((0.0, 1.0, 0.0), (1.0, 0.5, 0.0), (0.0, -1.0, 0.0), (0.3, 0.0, 0.9), (-2.0, 0.1, 7.0)):
        R.add((0.0, -5.0, 0.0) if d[1] <= 0 else (0.0, 20.0, 0.0), d)
    return R.done()


def recs_nonfinite():
    """hit_ray_cases' non-finite class on the panels: a NaN or an infinity in one component of the direction or
    of the origin.  Sky colours, mostly NaN."""
    R = Recs()
    bad = (math.nan, math.inf, -math.inf)
    for k in range(12):
        d = [0.3, -1.0, 0.2]
        o = [0.5 - 2.0 * d[0], 1.0 - 2.0 * d[1], 4.0 * (k % 4) - 2.0 * d[2]]
        (d if k % 2 == 0 else o)[k % 3] = bad[(k // 2) % 3]
        R.add(o, d)
    return R.done()


_panel = {}


def panel_classes():
    """{class: records (n, 7)} of the panel scene (every variant: the decoys are out of reach)."""
    if not _panel:
        with np.errstate(all="ignore"):
            _panel.update({
                "checker": recs_checker(), "noise": recs_noise(), "onb": recs_onb(), "metal": recs_metal(),
                "dielectric": recs_dielectric(), "lights": recs_lights(), "mixture": recs_mixture(),
                "miss": recs_miss(),
            })
            _panel["nonfinite"] = recs_nonfinite()
    return _panel


def mixed(n=None):
    """The panel classes one after the other (time-0 records only), tiled to n records."""
    allr = np.concatenate([r for c, r in panel_classes().items()])
    if n is None:
        return allr
    reps = (n + len(allr) - 1) // max(1, len(allr))
    return np.concatenate([allr] * max(1, reps))[:n]


# ------------------------------------------------------------------ small rooms
def _room_cam():
    return make_camera(v.vec3(0, 2, 12), v.vec3(0, 2, 0), v.vec3(0, 1, 0), 40, 1.0, 0, 1, 0, 1)


_rooms = {}


def rooms():
    """mix_rect / mix_sphere: a floor at y = 0, lambertian plates at y = 4 and y = 6, and the sampled light: a
    rect at y = 4 facing down, or a sphere of radius 1 at (0, 4, 0) with a small lambertian plate inside it.
    media: a floor, a box medium and a sphere medium under the gradient sky."""
    if _rooms:
        return _rooms
    white = g.make_lambertian(_c(0.73, 0.73, 0.73))
    red = g.make_lambertian(g.checker_texture(_c(0.65, 0.05, 0.05), _c(0.1, 0.1, 0.6)))
    lamp = g.make_diffuse_light(_c(15, 15, 15))
    floor = g.make_xz_rect(-8, 8, -8, 8, 0, white)
    beside = g.flip_normals(g.make_xz_rect(2, 4, -1, 1, 4, red))
    behind = g.flip_normals(g.make_xz_rect(-2, 2, -2, 2, 6, white))
    rect_light = g.flip_normals(g.make_xz_rect(-1, 1, -1, 1, 4, lamp))
    _rooms["mix_rect"] = g.make_scene([floor, beside, behind, rect_light], _room_cam(), g.black, light=rect_light)
    sph_light = g.make_sphere(v.vec3(0, 4, 0), 1.0, lamp)
    inside = g.make_xz_rect(-0.25, 0.25, -0.25, 0.25, 4, white)
    _rooms["mix_sphere"] = g.make_scene([floor, beside, behind, sph_light, inside], _room_cam(), g.black, light=sph_light)
    # mix_two: the rect light and a second, spherical one, as a light list of two different lights
    sph2 = g.make_sphere(v.vec3(5, 2, 0), 0.5, lamp)
    _rooms["mix_two"] = g.make_scene([floor, beside, behind, rect_light, sph2], _room_cam(), g.black,
                                     lights=[rect_light, sph2])
    _rooms["mix_two_single"] = g.make_scene([floor, beside, behind, rect_light, sph2], _room_cam(), g.black,
                                            light=rect_light)
    box_m = g.make_constant_medium(g.make_box(v.vec3(-1, 0, -1), v.vec3(1, 2, 1), white), 0.5, _c(0.9, 0.9, 0.9))
    sph_m = g.make_constant_medium(g.make_sphere(v.vec3(4, 1, 0), 1.0, white), 0.8, _c(0.2, 0.4, 0.9))
    metal = g.make_sphere(v.vec3(-4, 1, 0), 1.0, g.make_metal(_c(0.8, 0.8, 0.8), 0.2))
    _rooms["media"] = g.make_scene([floor, box_m, sph_m, metal], _room_cam(), g.sky_color)
    return _rooms


def oracle_room(oracle_mod, name):
    """The oracle's scene of a room; mix_two: its single-light twin with the oracle's list rule over the rect light
    and the sphere (the room's only sphere), in the list's order."""
    if name != "mix_two":
        return oracle_mod.build_scene(rooms()[name])
    o = oracle_mod.build_scene(rooms()["mix_two_single"])
    o.set_light_list([o.light_obj, o.spheres[-1]])
    return o


def recs_room_mixture():
    """Points under the light, on its plane beside it (pdf 0: the path ends), behind it, and (mix_sphere) inside
    the sphere light, where the solid angle's square root is NaN and the path ends."""
    R = Recs()
    for x in (0.0, 0.5, 2.0, -5.0, 7.5):
        for z in (0.0, 0.75, -3.0):
            R.down(x, z, y=0.0)                       # the floor: under the light and away from it
    for x in (2.5, 3.0, 3.75):
        for z in (0.0, 0.5, -0.75):
            R.up(x, z, y=4.0)                         # beside the light, on its plane
    for x in (0.0, 1.5, -1.75):
        for z in (0.0, 1.0):
            R.add((x - 3.0, 3.0, z), (1.0, 1.0, 0.0))  # behind the light (the plate at y = 6), past it
    for x in (0.0, 0.125, -0.25):
        for z in (0.0, 0.125):
            R.up(x, z, y=4.0, t=0.5)                  # inside the sphere light (the rect light's own face there)
    return R.done()


#: the media room's phase-function materials (the box medium's, the sphere medium's), in emit order: floor and
#: boundaries 0, then 1 and 2, the metal sphere 3
MEDIA_PHASE_MATS = (1, 2)
#: the record of recs_media whose scatter distance differs by one ulp of t between the device library's log and
#: the C library's (tests/test_gpu_scatter.py): the vertical ray of k = 6
MEDIUM_LOG_RECORD = 5 * 6 + 4


def recs_media():
    """Through, into (origin inside) and past the two media."""
    R = Recs()
    for k in range(16):
        y = 0.25 + 0.1 * k
        R.add((-6.0, y, 0.1 * k - 0.8), (1.0, 0.0, 0.0))                   # through the box, then the sphere
        R.add((0.0, y, 0.0), (1.0, 0.05 * k - 0.4, 0.1))                   # from inside the box
        R.add((4.0, 1.0, 0.0), (math.cos(0.4 * k), 0.2, math.sin(0.4 * k)))  # from inside the sphere
        R.add((-6.0, 3.0 + y, 0.0), (1.0, 0.0, 0.0))                       # past both
        R.add((0.1 * k - 0.8, 5.0, 0.3), (0.0, -1.0, 0.0))                  # down through the box to the floor
    return R.done()


# ------------------------------------------------------------------ SOLO sphere worlds
def solo_scene(n=24, noise=False):
    """A world that is one BVH of spheres (rt_scene_info.bvh_solo): the LDS extend, the point-record queue
    and the SOLO tail.  Sphere k at (4 (k % 8), 4 (k // 8), 0), radius 1, materials in turn; more than 256
    spheres take the leaf records out of LDS."""
    mats = [
        g.make_lambertian(_c(0.6, 0.5, 0.4)),
        g.make_lambertian(g.checker_texture(_c(0.2, 0.3, 0.1), _c(0.9, 0.9, 0.9))),
        g.make_metal(_c(0.7, 0.6, 0.5), 0.3),
        g.make_dielectric(1.5),
        g.make_diffuse_light(_c(2, 2, 2)),
        g.make_lambertian(g.noise_texture(4.0) if noise else _c(0.1, 0.7, 0.7)),
    ]
    sph = [g.make_sphere(v.vec3(4.0 * (k % 8), 4.0 * (k // 8), 0.0), 1.0, mats[k % len(mats)]) for k in range(n)]
    return g.make_scene([g.make_bvh_node(sph, 0, 1)], _room_cam(), g.sky_color,
                        perlin=_perlin.from_seed(PERLIN_SEED) if noise else None)


def recs_solo(n=24):
    R = Recs()
    for k in range(min(n, 24)):
        cx, cy = 4.0 * (k % 8), 4.0 * (k // 8)
        for dx, dy in ((0.0, 0.0), (0.5, 0.25), (-0.9, 0.1), (0.3, -0.95), (1.5, 0.0)):
            R.add((cx + dx, cy + dy, 8.0), (0.0, 0.0, -1.0))
            R.add((cx + dx * 0.5, cy + dy * 0.5, 0.0), (0.1, 0.2, 1.0))      # from inside
    return R.done()


# ------------------------------------------------------------------ the oracle's expectation
class Expect:
    """What one step must leave for records (rays, T, ctr, pix) at a depth, from the oracle's orc_step."""
    __slots__ = ("rows", "survive", "ray", "T", "ctr", "color", "t", "mat", "mtype")


def throughputs(n, depth):
    """T = 1 at depth 0 (the only legal one); deeper, varied finite throughputs so the forward order matters."""
    if depth == 0:
        return np.ones((n, 3))
    rng = np.random.default_rng([SEED, 7, n])
    return rng.uniform(0.05, 1.5, size=(n, 3))


def expect(osc, rays, depth, seed=SEED, smp=SMP, T=None, ctr=None, pix=None):
    import oracle
    n = len(rays)
    T = throughputs(n, depth) if T is None else T
    with np.errstate(all="ignore"):
        rows, ctr_out = osc.step(rays, depth, seed, smp, pix=pix, ctr_in=ctr)
        e = Expect()
        e.rows = rows
        e.survive = rows[:, oracle.STEP_KIND] == 1
        e.mtype = rows[:, oracle.STEP_MTYPE].astype(np.int32)
        e.ray = np.concatenate([rows[:, oracle.STEP_O], rows[:, oracle.STEP_D]], axis=1)
        a, ipdf = rows[:, oracle.STEP_A], rows[:, oracle.STEP_IPDF]
        # the device's documented forward order, from the oracle's parts
        lam = (T * a) * ipdf[:, None]
        e.T = np.where((e.mtype == MAT_LAMBERTIAN)[:, None], lam, np.where((e.mtype == MAT_METAL)[:, None], T * a, T))
        e.ctr = ctr_out
        e.color = T * rows[:, oracle.STEP_L]
        e.t = rows[:, oracle.STEP_T].copy()
        e.mat = rows[:, oracle.STEP_MAT].astype(np.int32)
    return e


def same_bits(a, b):
    """Elementwise bit equality of float64 arrays; two NaNs count as equal."""
    return hc.same_t(a, b)


def iterate_oracle(osc, rays, depth, seed=SEED, smp=SMP, T=None, ctr=None, pix=None):
    """orc_step iterated to the end of every path, the colour formed backwards as color() forms it: the
    weights are kept on a stack and applied from the last segment to the first."""
    import oracle
    n = len(rays)
    out = np.zeros((n, 3))
    pix = np.arange(n) if pix is None else pix
    ctr = np.zeros(n, dtype=np.uint32) if ctr is None else ctr
    with np.errstate(all="ignore"):
        for k in range(n):
            r, c, d, stack = rays[k:k + 1].copy(), ctr[k:k + 1], depth, []
            while True:
                rows, c = osc.step(r, d, seed, smp, pix=pix[k:k + 1], ctr_in=c)
                row = rows[0]
                if row[oracle.STEP_KIND] == 0:
                    L = row[oracle.STEP_L].copy()
                    break
                stack.append((int(row[oracle.STEP_MTYPE]), row[oracle.STEP_A].copy(), row[oracle.STEP_IPDF]))
                r = np.concatenate([row[oracle.STEP_O], row[oracle.STEP_D], [0.0]])[None, :]
                d += 1
            for mt, a, ipdf in reversed(stack):
                L = (0.0 + (a * L) * ipdf) if mt == MAT_LAMBERTIAN else a * L
            out[k] = L
    return out
