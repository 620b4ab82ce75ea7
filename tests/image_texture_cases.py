"""Shared by test_image_texture_host.py and test_gpu_image_texture.py: the image-texture test scenes, the
split-rect helper (an image-textured rect as nx*ny constant-textured sub-rects, which the oracle can hold),
and the oracle's first-hit samples on the textured spheres.  Texture colours are bytes, so k/255 is the same
f64 wherever it is formed.  Every shared result is computed once per session and returned read-only."""
import functools

import numpy as np

import feature_cases
from rtamd import image
from rtamd import scene as g
from rtamd import scenes
from rtamd import vec as v
from rtamd.camera import make_camera
from rtamd.scene import emit

SEED = 0x5EED0002


def byte_colour(rgb):
    """A colour given as three bytes, as the doubles an image texture returns for them."""
    return tuple(int(k) / 255.0 for k in rgb)


def formula_image(nx, ny, salt=0):
    """A deterministic nx x ny test image whose neighbouring texels all differ."""
    y, x = np.mgrid[0:ny, 0:nx]
    img = np.zeros((ny, nx, 3), dtype=np.uint8)
    img[..., 0] = (37 * x + 11 * y + 5 * salt + 20) % 256
    img[..., 1] = (91 * y + 23 * x + 7 * salt + 60) % 256
    img[..., 2] = (53 * (x + y) + 13 * salt + 100) % 256
    return img.reshape(-1)


def constant_image(rgb, nx, ny):
    """nx x ny texels all equal to the bytes rgb."""
    return np.tile(np.array(rgb, dtype=np.uint8), nx * ny)


# ---------------------------------------------------------------- split rects
def _with_texture(material, tex):
    if material.kind == "lambertian":
        return g.make_lambertian(tex)
    if material.kind == "metal":
        return g.make_metal(tex, material.args[1])
    if material.kind == "diffuse_light":
        return g.make_diffuse_light(tex)
    raise ValueError(material.kind)


def split_seams(a0, a1, b0, b1, nx, ny):
    """The in-plane seam coordinates of an nx x ny image on the rect [a0, a1] x [b0, b1]: columns change at
    u = m / nx, rows at v = 1 - (m + 0.001) / ny (row m lies below its seam: j = (1 - v) ny - 0.001 >= m).
    Returns (a_edges, b_edges), nx + 1 ascending and ny + 1 ascending values, the rect's own edges included;
    b_edges[k] .. b_edges[k + 1] is image row ny - 1 - k."""
    ua = [m / nx for m in range(1, nx)]
    vb = sorted(1.0 - (m + 0.001) / ny for m in range(1, ny))
    a_edges = [a0] + [a0 + u * (a1 - a0) for u in ua] + [a1]
    b_edges = [b0] + [b0 + w * (b1 - b0) for w in vb] + [b1]
    return a_edges, b_edges


def split_rect(rect, img):
    """The image-textured rect ``rect`` (a "rect" hitable whose material's texture is the image texture
    ``img``) as nx*ny rects of constant texture, one per texel, same axis, plane and material kind."""
    assert rect.kind == "rect" and img.kind == "image"
    axis, a0, a1, b0, b1, k, material = rect.args
    data, nx, ny = img.args
    tex = data.reshape(ny, nx, 3)
    a_edges, b_edges = split_seams(a0, a1, b0, b1, nx, ny)
    make = (g.make_xy_rect, g.make_xz_rect, g.make_yz_rect)[axis]
    out = []
    for row in range(ny):
        lo, hi = b_edges[ny - 1 - row], b_edges[ny - row]
        for col in range(nx):
            m = _with_texture(material, g.constant_texture(byte_colour(tex[row, col])))
            out.append(make(a_edges[col], a_edges[col + 1], lo, hi, k, m))
    return out


def split_rect_colour_at(subrects, a_edges, b_edges, nx, ny, a, b):
    """The colour of the sub-rect (split_rect's order) containing in-plane points (a, b): arrays in, (n, 3) out."""
    col = np.clip(np.searchsorted(np.array(a_edges), a, side="right") - 1, 0, nx - 1)
    band = np.clip(np.searchsorted(np.array(b_edges), b, side="right") - 1, 0, ny - 1)
    row = ny - 1 - band
    colours = np.array([r.args[6].args[0].args[0] for r in subrects]).reshape(ny, nx, 3)
    return colours[row, col]


# ---------------------------------------------------------------- test scenes
def _room_camera(nx, ny):
    return make_camera(v.vec3(278, 278, -800), v.vec3(278, 278, 0), v.vec3(0, 1, 0), 40, nx / ny, 0, 1, 0, 1)


def constant_room(nx, ny, mode):
    """GPU test 1's room.  mode "const": constant textures; "1x1" / "5x3": every constant replaced by an image
    of that size whose texels all equal the colour."""
    def tex(rgb):
        if mode == "const":
            return g.constant_texture(byte_colour(rgb))
        w, h = (1, 1) if mode == "1x1" else (5, 3)
        return g.make_image_texture(constant_image(rgb, w, h), w, h)

    white = g.make_lambertian(tex((186, 186, 186)))
    red = g.make_lambertian(tex((166, 13, 13)))
    green = g.make_lambertian(tex((31, 115, 38)))
    mirror = g.make_metal(tex((204, 153, 51)), 0.25)
    light = g.make_diffuse_light(tex((255, 255, 255)))
    patch = g.make_lambertian(g.checker_texture(tex((51, 77, 26)), tex((230, 230, 230))))
    objs = [
        g.flip_normals(g.make_yz_rect(0, 555, 0, 555, 555, green)),
        g.make_yz_rect(0, 555, 0, 555, 0, red),
        g.flip_normals(g.make_xz_rect(113, 443, 127, 432, 554, light)),
        g.flip_normals(g.make_xz_rect(0, 555, 0, 555, 555, white)),
        g.make_xz_rect(0, 555, 0, 555, 0, white),
        g.flip_normals(g.make_xy_rect(0, 555, 0, 555, 555, white)),
        g.make_xz_rect(30, 250, 20, 200, 1, patch),
        g.translate(g.rotate_y(g.make_box(v.vec3(0, 0, 0), v.vec3(140, 260, 140), white), 15), v.vec3(330, 0, 300)),
        g.translate(g.rotate_y(g.make_xy_rect(0, 160, 0, 200, 0, mirror), -25), v.vec3(60, 120, 380)),
        g.make_sphere(v.vec3(150, 90, 260), 70, g.make_lambertian(tex((64, 128, 230)))),
        g.make_sphere(v.vec3(420, 330, 200), 55, g.make_metal(tex((230, 200, 180)), 0.0)),
        g.make_moving_sphere(v.vec3(270, 60, 120), v.vec3(270, 95, 120), 0, 1, 45,
                             g.make_lambertian(tex((200, 60, 160)))),
        g.make_constant_medium(g.make_sphere(v.vec3(300, 420, 330), 80, white), 0.02, tex((240, 240, 250))),
    ]
    return g.make_scene(objs, _room_camera(nx, ny), g.sky_color)


#: GPU test 2's image sizes: floor, back wall, ceiling light, metal rect
RECT_IMAGES = {"floor": (4, 3), "back": (2, 2), "light": (2, 1), "mirror": (3, 2)}


def rect_room(nx, ny, split):
    """GPU test 2's rect-only room: image textures (split False) or their split_rect twins (split True)."""
    imgs = {name: g.make_image_texture(formula_image(w, h, salt), w, h)
            for salt, (name, (w, h)) in enumerate(sorted(RECT_IMAGES.items()))}
    # a light's bytes are its emission; keep them bright
    lw, lh = RECT_IMAGES["light"]
    imgs["light"] = g.make_image_texture(np.array([255, 240, 200, 200, 230, 255], dtype=np.uint8), lw, lh)

    def surface(rect, img, wrap=lambda r: r):
        return [wrap(r) for r in split_rect(rect, img)] if split else [wrap(rect)]

    red = g.make_lambertian(g.constant_texture(byte_colour((166, 13, 13))))
    green = g.make_lambertian(g.constant_texture(byte_colour((31, 115, 38))))
    white = g.make_lambertian(g.constant_texture(byte_colour((186, 186, 186))))
    objs = [g.flip_normals(g.make_yz_rect(0, 555, 0, 555, 555, green)), g.make_yz_rect(0, 555, 0, 555, 0, red)]
    objs += surface(g.make_xz_rect(113, 443, 127, 432, 554, g.make_diffuse_light(imgs["light"])), imgs["light"],
                    g.flip_normals)
    objs += [g.flip_normals(g.make_xz_rect(0, 555, 0, 555, 555, white))]
    objs += surface(g.make_xz_rect(0, 555, 0, 555, 0, g.make_lambertian(imgs["floor"])), imgs["floor"])
    objs += surface(g.make_xy_rect(0, 555, 0, 555, 555, g.make_lambertian(imgs["back"])), imgs["back"], g.flip_normals)
    objs += surface(g.make_xy_rect(0, 220, 0, 260, 0, g.make_metal(imgs["mirror"], 0.1)), imgs["mirror"],
                    lambda r: g.translate(g.rotate_y(r, -20), v.vec3(170, 60, 330)))
    return g.make_scene(objs, _room_camera(nx, ny), g.sky_color)


#: GPU test 3 / CPU test 6: the sphere image and frame
SPHERE_IMAGE = (8, 4)
SPHERE_FRAME = (32, 32, 4)                 # nx, ny, passes
SPHERE_TRANSLATE = (0.35, 0.1, -0.2)
#: (kind, centre(s), radius) of the three textured spheres, in object order
SPHERES = [("sphere", (-1.15, 0.0, 0.0), 0.55),
           ("moving", ((0.0, -0.15, 0.0), (0.0, 0.35, 0.0)), 0.5),
           ("translated", (0.9, 0.05, 0.1), 0.5)]


def sphere_image():
    return formula_image(SPHERE_IMAGE[0], SPHERE_IMAGE[1], salt=3)


def sphere_scene(nx, ny, textured):
    """Three spheres (plain, moving over the shutter 0..1, under a translate) in front of the sky: with the
    8x4 image on each (textured) or a constant colour each (the twin the oracle can hold)."""
    img = g.make_image_texture(sphere_image(), *SPHERE_IMAGE) if textured else None
    consts = [(200, 60, 60), (60, 200, 60), (60, 60, 200)]
    objs = []
    for (kind, c, r), rgb in zip(SPHERES, consts):
        m = g.make_lambertian(img if textured else g.constant_texture(byte_colour(rgb)))
        if kind == "sphere":
            objs.append(g.make_sphere(v.vec3(*c), r, m))
        elif kind == "moving":
            objs.append(g.make_moving_sphere(v.vec3(*c[0]), v.vec3(*c[1]), 0, 1, r, m))
        else:
            objs.append(g.translate(g.make_sphere(v.vec3(*c), r, m), v.vec3(*SPHERE_TRANSLATE)))
    cam = make_camera(v.vec3(0, 0.6, 4.2), v.vec3(0, 0.05, 0), v.vec3(0, 1, 0), 32, nx / ny, 0.05, 4.2, 0, 1)
    return g.make_scene(objs, cam, g.sky_color)


@functools.lru_cache(maxsize=None)
def sphere_samples(seed=SEED):
    """The oracle's first hits (trace_sample, cap 1) of the constant twin of sphere_scene, one row per camera
    sample in (pixel, pass) order: (pixel, pass, sphere index or -1 for a miss, u, v, base rgb) where u, v are
    rtamd.image.sphere_uv of the unit normal formed as the library forms it — the point o + d t on the
    instance-local ray, the centre at the camera ray's time — and base rgb is the constant twin's albedo
    (the sky colour for a miss)."""
    nx, ny, passes = SPHERE_FRAME
    sc = sphere_scene(nx, ny, False)
    o = emit(sc, feature_cases._recording_oracle())
    mats = sorted(o.materials)                          # one lambertian per sphere, in object order
    rows = np.zeros((nx * ny * passes, 8))
    k = 0
    for j in range(nx * ny):
        y, x = divmod(j, nx)
        for smp in range(passes):
            row = o.trace_sample(nx, ny, x, y, seed, smp, cap=1)[0]
            if row[6] == 0.0:
                rows[k] = (j, smp, -1, 0.0, 0.0) + tuple(o.sample(nx, ny, x, y, seed, smp))
                k += 1
                continue
            idx = mats.index(int(row[11]))
            kind, c, r = SPHERES[idx]
            org, d, t = row[0:3], row[3:6], row[7]
            if kind == "translated":
                org = org - np.array(SPHERE_TRANSLATE)
            pt = org + d * t
            if kind == "moving":
                time = feature_cases.camera_time(sc, seed, j, smp)
                c0, c1 = np.array(c[0]), np.array(c[1])
                cen = c0 + (c1 - c0) * ((time - 0.0) / (1.0 - 0.0))
            else:
                cen = np.array(c)
            n = (pt - cen) * (1.0 / r)
            u, w = image.sphere_uv(n)
            rows[k] = (j, smp, idx, float(u), float(w)) + tuple(o.tex_value(o.materials[int(row[11])][1], row[8:11]))
            k += 1
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def sphere_expected_albedo(seed=SEED):
    """(nx*ny, 3): the per-pass sums, in pass order, of the image's value at each sample's (u, v) — the sky
    colour where the camera ray misses."""
    nx, ny, passes = SPHERE_FRAME
    rows = sphere_samples(seed)
    hit = rows[:, 2] >= 0
    colour = rows[:, 5:8].copy()
    colour[hit] = image.lookup(sphere_image(), SPHERE_IMAGE[0], SPHERE_IMAGE[1], rows[hit, 3], rows[hit, 4])
    out = np.zeros((nx * ny, 3))
    for smp in range(passes):
        sel = rows[:, 1] == smp
        out[rows[sel, 0].astype(int)] = out[rows[sel, 0].astype(int)] + colour[sel]
    out.setflags(write=False)
    return out


def cornell_image_scene(nx, ny):
    return scenes.cornell_image(nx, ny)
