"""Triangles on the host (no GPU): rtamd.mesh — the NumPy restatement of include/rt.h's "triangles", the OBJ
reader and the generators — the add calls' refusals through the C ABI, and the HIP-free scene build on scenes
with triangles (tests/csrc/tri_check.cpp, compiled beside rt_build.cpp under AddressSanitizer and UBSan)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
from rtamd import _lib, mesh, scenes
from rtamd import scene as g

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scheme-raytrace_amd", "csrc")


def test_watertight_test_misses_no_ray_of_a_closed_mesh():
    """icosphere(2) from its centre and 200 interior points, rays aimed exactly at every vertex, edge midpoint
    and a seeded point on every edge: every ray hits.  The same rays through Möller–Trumbore are counted only."""
    rays, vs, fs = mc.watertight_rays()
    assert rays.shape[0] == 201 * (162 + 480 + 480)
    t, idx = mesh.hit(vs[fs], rays)
    missed = int((idx < 0).sum())
    mt_t, mt_idx = mc.moller_trumbore(vs[fs], rays)
    print("watertight: %d rays, %d missed; Moeller-Trumbore misses %d of them" % (len(rays), missed, int((mt_idx < 0).sum())))
    assert missed == 0
    assert (t > 0.3).all() and (t < 1.7).all()                    # the far side of a unit ball seen from within radius 0.6


def test_hit_rule_on_hand_cases():
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    rays = np.array([
        [0.25, 0.25, 1.0, 0, 0, -1.0, 0],       # through the inside, from the front: t = 1
        [0.25, 0.25, -2.0, 0, 0, 0.5, 0],       # from the back (two-sided), half-length direction: t = 4
        [0.0, 0.0, 1.0, 0, 0, -1.0, 0],         # a vertex: inclusive
        [0.5, 0.5, 1.0, 0, 0, -1.0, 0],         # the hypotenuse: inclusive
        [0.75, 0.75, 1.0, 0, 0, -1.0, 0],       # outside
        [-1.0, 0.25, 0.0, 1.0, 0, 0, 0],        # in the plane: a miss
        [0.25, 0.25, 0.0005, 0, 0, -1.0, 0],    # t below 0.001
        [0.25, 0.25, 1.0, 0, 0, 1.0, 0],        # behind the origin
        [0.25, 0.25, 1.0, 0, np.nan, -1.0, 0],  # a NaN passes no comparison
        [np.inf, 0.25, 1.0, 0, 0, -1.0, 0],
    ])
    t, idx = mesh.hit(tri, rays)
    assert idx.tolist() == [0, 0, 0, 0, -1, -1, -1, -1, -1, -1]
    assert t.tolist() == [1.0, 4.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0]
    # two coincident triangles: the first in list order keeps the hit
    t, idx = mesh.hit(np.concatenate([tri, tri]), rays[:1])
    assert idx.tolist() == [0]
    # the per-ray constants: the largest component, ties to the lower axis, the winding kept for a negative one
    kx, ky, kz, Sx, Sy, Sz = mesh.ray_constants(np.array([[1.0, 1.0, 0.5], [0.5, -2.0, 2.0], [0.0, 0.0, -4.0], [1.0, 2.0, -2.0]]))
    assert kz.tolist() == [0, 1, 2, 1]
    assert (kx.tolist(), ky.tolist()) == ([1, 0, 1, 2], [2, 2, 0, 0])
    assert Sz.tolist() == [1.0, -0.5, -0.25, 0.5] and Sx.tolist() == [1.0, -0.25, -0.0, -1.0]


def test_normal_and_uv_rules_on_hand_cases():
    tri = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    assert mesh.normal(tri).tolist() == [0.0, 0.0, 1.0]
    assert mesh.normal(tri[::-1]).tolist() == [0.0, 0.0, -1.0]
    n = mesh.normal(np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]))
    k = 1.0 / np.sqrt((1.0 + 1.0) + 1.0)
    assert n.tolist() == [k, k, k]
    uvs = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    u, v = mesh.uv(tri, uvs, np.array([[0.5, 1.0, 0.0], [2.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 0.0]]))
    assert u.tolist() == [0.25, 1.0, 0.0, 0.0] and v.tolist() == [0.25, 0.0, 1.0, 0.0]
    u, v = mesh.uv(tri, np.array([[0.25, 0.5], [0.75, 0.5], [0.25, 1.0]]), np.array([1.0, 2.0, 0.0]))
    assert (float(u), float(v)) == (0.5, 0.75)
    u, v = mesh.uv(tri, None, np.array([[0.5, 1.0, 0.0]]))
    assert u.tolist() == [0.0] and v.tolist() == [0.0]
    # rect_quad: the rect's normal (flips included) and its u, v at the corners
    for axis, want in ((0, [0, 0, 1.0]), (1, [0, 1.0, 0]), (2, [1.0, 0, 0])):
        for flip in (False, True):
            vs, fs, q = mesh.rect_quad(axis, 1.0, 3.0, 2.0, 6.0, 5.0, flip)
            assert mesh.normal(vs[fs]).tolist() == [[(-x if flip else x) + 0.0 for x in want]] * 2
            ia, ib = (1 if axis == 2 else 0), (1 if axis == 0 else 2)
            assert np.array_equal(q[:, 0], (vs[:, ia] - 1.0) / 2.0) and np.array_equal(q[:, 1], (vs[:, ib] - 2.0) / 4.0)


def test_generators():
    vs, fs = mesh.icosphere(2, radius=2.0, center=(1.0, 2.0, 3.0))
    assert vs.shape == (162, 3) and fs.shape == (320, 3) and fs.dtype == np.int32
    assert np.allclose(np.linalg.norm(vs - [1.0, 2.0, 3.0], axis=1), 2.0, rtol=0, atol=1e-14)
    edges = np.sort(np.concatenate([fs[:, [0, 1]], fs[:, [1, 2]], fs[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()                                     # closed: every edge in exactly two faces
    n, c = mesh.normal(vs[fs]), vs[fs].mean(axis=1) - [1.0, 2.0, 3.0]
    assert (np.einsum("ij,ij->i", n, c) > 0).all()                 # outward
    assert mesh.icosphere(5)[1].shape == (20480, 3)
    bv, bf, bu = mesh.box((0, 0, 0), (1, 2, 3))
    assert bv.shape == (24, 3) and bf.shape == (12, 3) and bu.shape == (24, 2)
    assert (np.einsum("ij,ij->i", mesh.normal(bv[bf]), bv[bf].mean(axis=1) - [0.5, 1.0, 1.5]) > 0).all()
    sc = scenes.SCENES["cornell_mesh"](16, 16)
    assert sum(lf.tris.shape[0] for lf in mc.leaves_of(sc)) == 36
    assert [o.kind for o in scenes.SCENES["cornell_lifted"](16, 16).obj_list] == ["flip", "rect", "flip", "flip", "rect", "flip",
                                                                                 "translate", "translate"]


def test_read_obj_round_trips(tmp_path):
    p = tmp_path / "quad.obj"
    p.write_text("# a quad and a triangle\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\n"
                 "f 1/1/1 2/2/1 3/3/1 4/4/1\nv 2 0 0.5\nf -1/1 -4/3 -3/3\n")
    vs, fs, uvs = mesh.read_obj(str(p))
    # the polygon fanned from its first corner; negative indices; (v 2, vt 3) is a new vertex, (v 3, vt 3) a shared one
    assert fs.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 2]]
    assert vs.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0.5], [1, 0, 0]]
    assert uvs.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1], [0, 0], [1, 1]]
    # without vt (v and v//vn corners): no uvs; vertices shared by index
    q = tmp_path / "plain.obj"
    q.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvn 1 0 0\nf 1 2 3\nf 1//1 3//1 4//1\nf -4 -3 -1\n")
    vs, fs, uvs = mesh.read_obj(str(q))
    assert uvs is None and vs.shape == (4, 3) and fs.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3]]
    # a generated mesh written out and read back: the same arrays
    iv, jf = mesh.icosphere(1)
    r = tmp_path / "ball.obj"
    r.write_text("".join("v %r %r %r\n" % tuple(float(x) for x in v) for v in iv) +
                 "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in f) for f in jf))
    vs, fs, uvs = mesh.read_obj(str(r))
    order = np.unique(jf.ravel(), return_index=True)[1]
    first_use = jf.ravel()[np.sort(order)]                         # read_obj numbers vertices by first use
    assert np.array_equal(vs, iv[first_use]) and np.array_equal(vs[fs], iv[jf]) and uvs is None
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="out of range"):
        mesh.read_obj(str(bad))


def test_constructors_refuse_bad_triangles_and_the_oracle_refuses_triangles(oracle_mod):
    red = g.make_lambertian(g.constant_texture((0.65, 0.05, 0.05)))
    with pytest.raises(TypeError):
        g.make_triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), "not a material")
    with pytest.raises(ValueError, match="not finite"):
        g.make_triangle((0, 0, 0), (1, float("nan"), 0), (0, 1, 0), red)
    with pytest.raises(ValueError, match="degenerate"):
        g.make_triangle((0, 0, 0), (1, 1, 1), (2, 2, 2), red)
    with pytest.raises(ValueError, match="face 1 is degenerate"):
        g.make_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2), (0, 1, 1)], red)
    with pytest.raises(ValueError, match="out of range"):
        g.make_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 3)], red)
    with pytest.raises(ValueError, match="uvs"):
        g.make_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2)], red, uvs=[(0, 0)])
    sc = mc.scene_of("one_triangle")
    with pytest.raises(NotImplementedError, match="triangles are not restated"):
        oracle_mod.build_scene(sc)
    oracle_mod.build_scene(scenes.SCENES["cornell_lifted"](8, 8))  # the rect twin of cornell_mesh: the oracle holds it


def test_add_calls_refuse_their_arguments_without_gpu():
    """rt_add_triangle / rt_add_mesh check their arguments before the handle, so no context is needed."""
    L = _lib.lib()
    out = ctypes.c_int(0)
    dv = _lib.dvec
    a, b, c = dv((0, 0, 0)), dv((1, 0, 0)), dv((0, 1, 0))
    err = lambda: L.rt_last_error().decode()
    assert L.rt_add_triangle(424242, a, b, c, 0, None) != 0 and "null" in err()
    assert L.rt_add_triangle(424242, a, None, c, 0, ctypes.byref(out)) != 0 and "null vertex" in err()
    assert L.rt_add_triangle(424242, a, dv((1, float("inf"), 0)), c, 0, ctypes.byref(out)) != 0 and "not finite" in err()
    assert L.rt_add_triangle(424242, a, b, dv((2, 0, 0)), 0, ctypes.byref(out)) != 0 and "degenerate" in err()
    assert L.rt_add_triangle(424242, a, b, c, 0, ctypes.byref(out)) != 0 and "invalid scene handle" in err()
    verts = (ctypes.c_double * 12)(0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1)
    i32 = ctypes.c_int32 * 6
    assert L.rt_add_mesh(424242, None, 4, i32(0, 1, 2, 0, 1, 3), 2, None, 0, ctypes.byref(out)) != 0 and "null" in err()
    assert L.rt_add_mesh(424242, verts, 4, None, 2, None, 0, ctypes.byref(out)) != 0 and "null" in err()
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 0, 1, 3), 2, None, 0, None) != 0 and "null" in err()
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 0, 1, 4), 2, None, 0, ctypes.byref(out)) != 0
    assert "face 1" in err() and "out of range" in err()
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 0, -1, 3), 2, None, 0, ctypes.byref(out)) != 0 and "out of range" in err()
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 3, 1, 1), 2, None, 0, ctypes.byref(out)) != 0
    assert "face 1" in err() and "degenerate" in err()
    nanv = (ctypes.c_double * 12)(0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, float("nan"))
    assert L.rt_add_mesh(424242, nanv, 4, i32(0, 1, 2, 0, 1, 3), 2, None, 0, ctypes.byref(out)) != 0
    assert "face 1" in err() and "not finite" in err()
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 0, 1, 3), 0, None, 0, ctypes.byref(out)) != 0 and "at least 1" in err()
    assert L.rt_add_mesh(424242, verts, 0, i32(0, 1, 2, 0, 1, 3), 2, None, 0, ctypes.byref(out)) != 0 and "at least 1" in err()
    uvs = (ctypes.c_double * 8)(0, 0, 1, 0, 0, 1, float("inf"), 1)
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 0, 1, 3), 2, uvs, 0, ctypes.byref(out)) != 0
    assert "face 1" in err() and "texture coordinate" in err()
    assert L.rt_add_mesh(424242, verts, 4, i32(0, 1, 2, 0, 1, 3), 2, None, 0, ctypes.byref(out)) != 0 and "invalid scene handle" in err()


def test_abi_announces_triangles():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt) and re.search(r"#define\s+RT_HAS_TRIANGLES\s+1\b", txt)
    assert "rt_add_triangle" in _lib.EXPORTED and "rt_add_mesh" in _lib.EXPORTED
    assert [n for n, _ in _lib.RtTreeInfo._fields_][12] == "tri_leaves" and ctypes.sizeof(_lib.RtTreeInfo) == 64
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rt_add_triangle" in doc and "rt_add_mesh" in doc and "RT_HAS_TRIANGLES" in doc


@pytest.fixture(scope="module")
def tri_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tri") / "tri_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "csrc", "tri_check.cpp"), os.path.join(CSRC, "rt_build.cpp")])
    return exe


def test_scene_build_with_triangles_under_sanitizers(tri_check):
    """Triangles under no chain, under translate and under rotate-y + translate: vertices in their leaf boxes,
    every leaf reached once, tri_leaves right, the build deterministic, the commit's refusals; no sanitizer report."""
    r = subprocess.run([tri_check], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout)
    assert res["ok"] and res["error"] == ""
    assert res["tris"] == 3 * 2 * 24 * 24 and res["tri_leaves"] == res["tris"] and res["n_tri"] == res["tris"]
    assert res["n_gleaf"] == res["tris"] + 22                      # with the 21 spheres and the rect
    assert res["outside"] == 0 and res["reach_bad"] == 0 and res["tri_ids_bad"] == 0 and res["normals_bad"] == 0
    assert res["same_threads"] and res["same_again"]
    assert res["single_ok"] and res["single_tri_leaves"] == 1 and res["single_n_gleaf"] == 1 and res["single_bad"] == 0
    for key in ("with_curve", "with_klein", "with_medium"):
        assert "cannot hold a curve, a Klein set or a constant medium" in res[key], (key, res[key])
    assert "boundary" in res["boundary"] and "light-sampling target" in res["light"] and "not finite" in res["far"]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr.strip() == ""
