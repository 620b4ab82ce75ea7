"""Image textures without a GPU: the header and exports, the ABI's refusals, the lookup rule against a scalar
restatement, the PPM reader, the split-rect helper the GPU parity test relies on, and the stability of the
sphere case's texels under ulp-sized changes of u, v (which licenses the GPU test's allowance: the device's
atan2 and asin are its own library's, not the host's).  The committed-scene refusal needs a device to commit
a scene; it is checked in test_gpu_image_texture.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import image_texture_cases as ic
from rtamd import _lib, image, render
from rtamd import scene as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. header and exports
def test_header_announces_image_textures_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt)
    assert re.search(r"#define\s+RT_HAS_IMAGE_TEXTURE\s+1\b", txt)
    assert "rt_add_texture_image" in _lib.EXPORTED
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "rt_add_texture_image" in {line.split()[-1] for line in out.splitlines() if line.strip()}


# ------------------------------------------------------------------ 2. refusals
def test_add_texture_image_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    out = ctypes.c_int(-7)
    px = (ctypes.c_uint8 * 12)()
    assert L.rt_add_texture_image(424242, None, 2, 2, ctypes.byref(out)) != 0
    assert b"null" in L.rt_last_error()
    assert L.rt_add_texture_image(424242, px, 2, 2, None) != 0
    assert b"null" in L.rt_last_error()
    for nx, ny in ((0, 2), (2, 0), (-1, 2), (2, -3)):
        assert L.rt_add_texture_image(424242, px, nx, ny, ctypes.byref(out)) != 0
        assert b"at least 1" in L.rt_last_error()
    # nx*ny > 2^26: refused on the sizes alone (the pointer is never read)
    assert L.rt_add_texture_image(424242, px, 8193, 8192, ctypes.byref(out)) != 0
    assert b"2^26" in L.rt_last_error()
    assert L.rt_add_texture_image(424242, px, 1 << 30, 1 << 30, ctypes.byref(out)) != 0
    assert b"2^26" in L.rt_last_error()
    assert L.rt_add_texture_image(424242, px, 2, 2, ctypes.byref(out)) != 0
    assert b"invalid scene" in L.rt_last_error()
    assert out.value == -7


def test_python_constructor_checks_its_data():
    with pytest.raises(ValueError):
        g.make_image_texture(bytes(11), 2, 2)
    with pytest.raises(ValueError):
        g.make_image_texture(bytes(0), 0, 2)
    with pytest.raises(TypeError):
        g.make_image_texture(np.zeros(12, dtype=np.float64), 2, 2)
    t = g.make_image_texture(bytes(range(12)), 2, 2)
    assert t.kind == "image" and t.args[1:] == (2, 2) and t.args[0].tolist() == list(range(12))
    # a checker takes an image as a child
    assert g.checker_texture(t, g.constant_texture((0.5, 0.5, 0.5))).kind == "checker"


def test_oracle_builder_refuses_image_textures_clearly(oracle_mod):
    from rtamd.camera import make_camera
    t = g.make_image_texture(bytes(12), 2, 2)
    sc = g.make_scene([g.make_sphere((0, 0, 0), 1, g.make_lambertian(t))],
                      make_camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 40, 1.0, 0, 1, 0, 1), g.sky_color)
    with pytest.raises(NotImplementedError, match="image textures"):
        oracle_mod.build_scene(sc)


# ------------------------------------------------------------------ 3. the lookup rule
def _scalar_lookup(data, nx, ny, u, v):
    """The rule of include/rt.h ("image textures"), one sample, scalar Python floats (IEEE f64)."""
    i = u * float(nx)
    j = (1.0 - v) * float(ny) - 0.001
    if not (i >= 0.0):
        i = 0.0
    if not (j >= 0.0):
        j = 0.0
    if i > float(nx - 1):
        i = float(nx - 1)
    if j > float(ny - 1):
        j = float(ny - 1)
    ii, jj = int(math.floor(i)), int(math.floor(j))
    k = 3 * (ii + nx * jj)
    return (int(data[k]) / 255.0, int(data[k + 1]) / 255.0, int(data[k + 2]) / 255.0)


def _lookup_cases(nx, ny):
    rng = np.random.default_rng(20240611)
    uv = [tuple(p) for p in rng.uniform(-0.25, 1.25, size=(2000, 2))]
    uv += [tuple(p) for p in rng.uniform(0.0, 1.0, size=(2000, 2))]
    inf, nan = float("inf"), float("nan")
    uv += [(-0.5, 0.3), (-1e-300, 0.3), (1.0, 0.3), (0.0, 0.3), (np.nextafter(1.0, 0.0), 0.3),   # u < 0, u = 1
           (0.3, 0.0), (0.3, 1.0), (0.3, -0.0), (0.3, 2.0), (0.3, -2.0)]                            # v = 0, v = 1
    for m in range(0, ny + 1):                       # v one ulp either side of every row seam, and on it
        seam = 1.0 - (m + 0.001) / ny
        uv += [(0.3, seam), (0.3, float(np.nextafter(seam, 2.0))), (0.3, float(np.nextafter(seam, -2.0)))]
    for m in range(0, nx + 1):                       # and u around the column seams
        seam = m / nx
        uv += [(seam, 0.4), (float(np.nextafter(seam, 2.0)), 0.4), (float(np.nextafter(seam, -2.0)), 0.4)]
    specials = [nan, inf, -inf, 0.25]
    uv += [(a, b) for a in specials for b in specials]
    return uv


@pytest.mark.parametrize("nx,ny", [(5, 3), (1, 1)])
def test_lookup_matches_the_scalar_rule_bit_for_bit(nx, ny):
    data = ic.formula_image(nx, ny, salt=1)
    uv = _lookup_cases(nx, ny)
    u = np.array([p[0] for p in uv])
    v = np.array([p[1] for p in uv])
    got = image.lookup(data, nx, ny, u, v)
    assert got.shape == (len(uv), 3) and got.dtype == np.float64
    want = np.array([_scalar_lookup(data, nx, ny, float(a), float(b)) for a, b in uv])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the named edge cases land where the rule says
    tex = data.reshape(ny, nx, 3) / 255.0
    assert np.array_equal(image.lookup(data, nx, ny, 0.3, 0.0), tex[ny - 1, int(0.3 * nx)])      # v = 0: last row
    assert np.array_equal(image.lookup(data, nx, ny, 0.3, 1.0), tex[0, int(0.3 * nx)])           # j = -0.001: row 0
    assert np.array_equal(image.lookup(data, nx, ny, 1.0, 0.3), image.lookup(data, nx, ny, 2.0, 0.3))
    assert np.array_equal(image.lookup(data, nx, ny, float("nan"), float("nan")), tex[0, 0])
    assert np.array_equal(image.lookup(data, nx, ny, float("inf"), float("inf")), tex[0, nx - 1])       # j = -inf
    assert np.array_equal(image.lookup(data, nx, ny, float("-inf"), float("-inf")), tex[ny - 1, 0])     # j = +inf
    # shapes: arrays in, (..., 3) out
    assert image.lookup(data, nx, ny, np.zeros((4, 2)), np.zeros((4, 2))).shape == (4, 2, 3)
    assert image.lookup(bytes(data), nx, ny, 0.5, 0.5).shape == (3,)


def test_uv_rules():
    u, v = image.rect_uv(np.array([10.0, 30.0]), np.array([5.0, 25.0]), 10, 50, 5, 45)
    assert u.tolist() == [0.0, 0.5] and v.tolist() == [0.0, 0.5]
    n = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 1e-300], [0.0, 1.0, 0.0], [0.0, -1.0000000001, 0.0], [0.0, 0.0, 1.0]])
    u, v = image.sphere_uv(n)
    assert u[0] == 0.5 and abs(u[1]) < 1e-15 and abs(u[4] - 0.25) < 1e-15
    assert v[0] == 0.5 and v[2] == 1.0 and v[3] == 0.0
    phi, theta = math.atan2(0.3, -0.2), math.asin(0.6)
    u, v = image.sphere_uv(np.array([-0.2, 0.6, 0.3]))
    assert u == 1.0 - (phi + math.pi) / (2.0 * math.pi) and v == (theta + math.pi / 2.0) / math.pi


# ------------------------------------------------------------------ 4. PPM round trips
def test_read_ppm_round_trips_p6_and_p3_with_comments(tmp_path):
    nx, ny = 5, 3
    data = ic.formula_image(nx, ny, salt=2)
    data[0:3] = (10, 32, 35)                       # whitespace and '#' bytes in the raster must not matter
    p6 = tmp_path / "a.ppm"
    p6.write_bytes(b"P6\n# a comment line\n%d %d\n255\n" % (nx, ny) + data.tobytes())
    got, gx, gy = image.read_ppm(str(p6))
    assert (gx, gy) == (nx, ny) and got.dtype == np.uint8 and np.array_equal(got, data)
    p3 = tmp_path / "b.ppm"
    rows = data.reshape(ny, nx * 3)
    p3.write_text("P3\n# made by a test\n%d %d # size\n255\n" % (nx, ny) +
                  "\n".join(" ".join(str(int(k)) for k in r) + " # row" for r in rows) + "\n")
    got, gx, gy = image.read_ppm(str(p3))
    assert (gx, gy) == (nx, ny) and np.array_equal(got, data)
    bad = tmp_path / "c.ppm"
    bad.write_bytes(b"P6\n2 2\n65535\n" + bytes(24))
    with pytest.raises(ValueError, match="maxval"):
        image.read_ppm(str(bad))
    bad.write_bytes(b"P6\n2 2\n255\n" + bytes(11))
    with pytest.raises(ValueError, match="truncated"):
        image.read_ppm(str(bad))


def test_read_ppm_reads_what_the_renderer_writes(tmp_path):
    """Renderer.save_as_ppm's writer (render.write_ppm: P3, rows top-down from the y-up image) needs no GPU."""
    nx, ny = 4, 3
    img = ic.formula_image(nx, ny, salt=5)                                  # y-up rows, as Renderer.image
    path = str(tmp_path / "r.ppm")
    render.write_ppm(path, img, nx, ny)
    got, gx, gy = image.read_ppm(path)
    assert (gx, gy) == (nx, ny)
    assert np.array_equal(got.reshape(ny, nx, 3), img.reshape(ny, nx, 3)[::-1])   # file order: top row first
    # and a texture takes it as it is
    assert g.make_image_texture(got, gx, gy).kind == "image"


# ------------------------------------------------------------------ 5. the split-rect helper
@pytest.mark.parametrize("axis,nx,ny", [(1, 4, 3), (0, 2, 2), (1, 2, 1), (0, 3, 2), (2, 5, 3), (1, 1, 1)])
def test_split_rect_agrees_with_lookup(axis, nx, ny):
    a0, a1, b0, b1, k = 113.0, 443.0, 127.0, 432.0, 554.0
    img = g.make_image_texture(ic.formula_image(nx, ny, salt=axis), nx, ny)
    make = (g.make_xy_rect, g.make_xz_rect, g.make_yz_rect)[axis]
    rect = make(a0, a1, b0, b1, k, g.make_metal(img, 0.25))
    subs = ic.split_rect(rect, img)
    assert len(subs) == nx * ny
    a_edges, b_edges = ic.split_seams(a0, a1, b0, b1, nx, ny)
    # the sub-rects tile the rect: same axis, plane and material kind, seams where the rule puts them
    for row in range(ny):
        for col in range(nx):
            s = subs[row * nx + col]
            assert s.kind == "rect" and s.args[0] == axis and s.args[5] == k
            assert s.args[6].kind == "metal" and s.args[6].args[1] == 0.25 and s.args[6].args[0].kind == "constant"
            assert (s.args[1], s.args[2]) == (a_edges[col], a_edges[col + 1])
            assert (s.args[3], s.args[4]) == (b_edges[ny - 1 - row], b_edges[ny - row])
    assert a_edges[0] == a0 and a_edges[-1] == a1 and b_edges[0] == b0 and b_edges[-1] == b1
    for m in range(1, nx):
        assert a_edges[m] == a0 + (m / nx) * (a1 - a0)
    for m in range(1, ny):
        assert b_edges[ny - m] == b0 + (1.0 - (m + 0.001) / ny) * (b1 - b0)
    # 10^5 random in-plane points: the containing sub-rect has lookup's colour, away from the seams
    rng = np.random.default_rng(7 + axis)
    a = rng.uniform(a0, a1, 100000)
    b = rng.uniform(b0, b1, 100000)
    u, v = image.rect_uv(a, b, a0, a1, b0, b1)
    useam = np.array([m / nx for m in range(1, nx)] or [np.inf])
    vseam = np.array([1.0 - (m + 0.001) / ny for m in range(1, ny)] or [np.inf])
    near = (np.abs(u[:, None] - useam[None, :]).min(axis=1) <= 1e-12) | \
           (np.abs(v[:, None] - vseam[None, :]).min(axis=1) <= 1e-12)
    print("split_rect %dx%d axis %d: %d of %d points left out (within 1e-12 of a seam)" % (nx, ny, axis, near.sum(), a.size))
    assert near.sum() <= 10
    want = image.lookup(img.args[0], nx, ny, u, v)
    got = ic.split_rect_colour_at(subs, a_edges, b_edges, nx, ny, a, b)
    assert np.array_equal(got[~near], want[~near])


# ------------------------------------------------------------------ 6. stability of the sphere case
def _ulp_shift(x, k):
    """x moved by k units in the last place (x > 0 finite)."""
    return (x.view(np.int64) + k).view(np.float64)


def test_sphere_case_texels_are_stable_under_4_ulp(oracle_mod):
    """GPU test 3 compares the device's u, v (its own atan2 / asin) with NumPy's: no sample of that test may
    sit within 4 ulp of a texel seam in u or v.  If one does, the case (seed, image size) is changed here."""
    nx, ny = ic.SPHERE_IMAGE
    rows = ic.sphere_samples()
    hit = rows[:, 2] >= 0
    per_sphere = [int((rows[:, 2] == k).sum()) for k in range(len(ic.SPHERES))]
    print("sphere case: %d samples, hits per sphere %s" % (rows.shape[0], per_sphere))
    assert min(per_sphere) >= 50, per_sphere               # every kind of sphere is seen
    u = np.ascontiguousarray(rows[hit, 3])
    v = np.ascontiguousarray(rows[hit, 4])
    assert (u > 0.0).all() and (u < 1.0).all() and (v > 0.0).all() and (v < 1.0).all()
    # the moving sphere's samples see different times (the shutter is open)
    base = image.texel_index(nx, ny, u, v)
    assert len(set(zip(base[0].tolist(), base[1].tolist()))) >= nx * ny // 2     # the image is really sampled
    moved = 0
    for du in range(-4, 5):
        for dv in range(-4, 5):
            ii, jj = image.texel_index(nx, ny, _ulp_shift(u, du), _ulp_shift(v, dv))
            moved += int(((ii != base[0]) | (jj != base[1])).sum())
    assert moved == 0
