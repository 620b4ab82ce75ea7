"""Per-vertex shading normals on the host (no GPU): rtamd.mesh.shading_normal — the NumPy restatement of
include/rt.h's "shading normals" — and the helpers around it, the OBJ reader's vn, rt_add_mesh_normals' refusals
through the C ABI, the HIP-free scene build on meshes with normals (tests/csrc/smooth_check.cpp, compiled beside
rt_build.cpp under AddressSanitizer and UBSan), and smooth_cases.scatter pinned to the oracle's orc_step."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import smooth_cases as sm
from rtamd import _lib, mesh, scenes
from rtamd import scene as g
from rtamd import vec as v
from rtamd.camera import make_camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scheme-raytrace_amd", "csrc")


# ------------------------------------------------------------------ 1. the restatement
def test_shading_normal_on_hand_cases():
    tri = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    k = 1.0 / np.sqrt((1.0 + 1.0) + 0.0)
    ns = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    # at a vertex: that vertex's normal
    got = mesh.shading_normal(tri, ns, tri)
    assert got.tolist() == ns.tolist()
    # at the midpoint of the edge v0 v1 (b1 = 0.5, b2 = 0): the normalised sum of two perpendicular unit normals
    got = mesh.shading_normal(tri, ns, np.array([1.0, 0.0, 0.0]))
    assert got.tolist() == [0.5 * (1.0 / np.sqrt(0.5)), 0.0, 0.5 * (1.0 / np.sqrt(0.5))]
    assert np.allclose(got, [k, 0.0, k], rtol=0, atol=1e-15)
    # the vertex normals are made unit first, as the add call makes them
    assert mesh.shading_normal(tri, ns * np.array([[3.0], [0.25], [7.0]]), tri).tolist() == ns.tolist()
    # vectorised over points of any shape
    pts = np.array([[[0.5, 1.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 2.0, 0.0], [0.0, 0.0, 0.0]]])
    out = mesh.shading_normal(tri, ns, pts)
    assert out.shape == (2, 2, 3)
    assert out[1, 0].tolist() == [0.0, 0.5 * (1.0 / np.sqrt(0.5)), 0.5 * (1.0 / np.sqrt(0.5))] and out[1, 1].tolist() == [0.0, 0.0, 1.0]
    b1, b2 = mesh.barycentrics(tri, pts)
    assert b1.tolist() == [[0.25, 0.5], [0.0, 0.0]] and b2.tolist() == [[0.25, 0.0], [0.5, 0.0]]


def test_equal_normals_come_back_bitwise():
    rng = np.random.RandomState(3)
    tri = np.array([[-1.0, 0.3, -0.5], [1.25, 0.25, -0.25], [0.1, 0.5, 1.5]])
    b = rng.dirichlet((1.0, 1.0, 1.0), 500)
    pts = np.concatenate([b @ tri, tri, rng.uniform(-3, 3, (100, 3))])          # inside, the vertices, anywhere
    for ax in range(3):
        for sgn in (1.0, -1.0):
            for zero in (0.0, -0.0):
                n0 = np.full(3, zero)
                n0[ax] = sgn
                got = mesh.shading_normal(tri, np.array([n0, n0, n0]), pts)
                assert (got == n0).all()                                       # (== : a zero of either sign passes)
                assert (got[:, ax] == sgn).all()
    n0 = mesh.unit_normals(np.array([0.3, -0.7, 0.2]))                            # an oblique unit normal too
    got = mesh.shading_normal(tri, np.array([n0, n0, n0]), pts)
    assert np.abs(got - n0).max() <= 2.0 ** -52                                   # (renormalised: q rounds beside 1)


def test_opposite_normals_fall_back_to_the_geometric_normal():
    tri = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    up, down = [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]
    # s = n0 + (n1 - n0) * 0.5 = 0 at the midpoint of v0 v1: q = 0, the geometric normal
    got = mesh.shading_normal(tri, np.array([up, down, up]), np.array([[1.0, 0.0, 0.0], [0.5, 0.0, 0.0]]))
    assert got[0].tolist() == mesh.normal(tri).tolist() == [0.0, 0.0, 1.0]
    assert got[1].tolist() == [0.0, 0.0, 1.0]                                    # (b1 = 0.25: s = (0, 0, 0.5))
    got = mesh.shading_normal(tri[::-1], np.array([up, down, up]), np.array([1.0, 2.0, 0.0]))   # v2 v1 v0: b1 = 0.5 too
    assert got.tolist() == [0.0, 0.0, -1.0]
    # a point so far away that q overflows: the geometric normal as well
    far = mesh.shading_normal(tri, np.array([up, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([1e200, 1e200, 0.0]))
    assert far.tolist() == [0.0, 0.0, 1.0]


# ------------------------------------------------------------------ 2. the sphere bound
@pytest.mark.parametrize("level,geo_median", [(1, 0.13), (3, 0.033)])
def test_radial_normals_give_the_sphere_normal(level, geo_median):
    """Radial vertex normals interpolated by the rule against unit(pt - c): at most 1e-12 (1000 x the 1.1e-15
    measured with NumPy); the geometric normal is off by more than 0.01 in the median on the same hits."""
    c = np.array((190.0, 91.0, 190.0))
    vs, fs, pt, idx = sm.sphere_hits(level)
    assert len(pt) >= 5000
    ns = mesh.radial_normals(vs, c)
    got = sm.shading_normals_at(vs, fs, ns, pt, idx)
    want = mesh.unit_normals(pt - c)
    dev = np.abs(got - want).max(axis=1)
    geo = np.abs(mesh.normal(vs[fs])[idx] - want).max(axis=1)
    print("icosphere(%d): %d hits, shading normal off by at most %.3e; geometric normal median %.4f max %.4f"
          % (level, len(pt), dev.max(), np.median(geo), geo.max()))
    assert dev.max() <= 1e-12
    assert np.median(geo) > 0.01
    assert 0.5 * geo_median < np.median(geo) < 2.0 * geo_median                  # (the issue's own measurement)


# ------------------------------------------------------------------ 3. vertex_normals
def test_vertex_normals_of_an_icosphere_are_radial():
    vs, fs = mesh.icosphere(2, radius=2.0, center=(1.0, 2.0, 3.0))
    got = mesh.vertex_normals(vs, fs)
    want = mesh.radial_normals(vs, (1.0, 2.0, 3.0))
    by_angle = mesh.vertex_normals(vs, fs, weights="angle")
    # (plain angle weights measure 8.9e-3 here: the default weights are Max's, exact for vertices on a sphere)
    print("vertex_normals on icosphere(2): max deviation from radial %.3e; with plain angle weights %.3e"
          % (np.abs(got - want).max(), np.abs(by_angle - want).max()))
    assert np.abs(got - want).max() <= 1e-3
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-15
    # a flat quad: every vertex gets the face normal
    qv, qf, _ = mesh.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0))
    assert mesh.vertex_normals(qv, qf).tolist() == [[0.0, 0.0, 1.0]] * 4
    # check_normals: what the add call refuses
    mesh.check_normals(want, fs)
    bad = want.copy()
    bad[fs[7, 1]] = 0.0
    first = int(np.nonzero((fs == fs[7, 1]).any(axis=1))[0][0])                  # the first face that uses the vertex
    with pytest.raises(ValueError, match="m: face %d has a vertex normal that has zero" % first):
        mesh.check_normals(bad, fs, "m")
    bad[fs[7, 1]] = (0.0, np.nan, 1.0)
    with pytest.raises(ValueError, match="not finite"):
        mesh.check_normals(bad, fs)
    red = g.make_lambertian(g.constant_texture((0.65, 0.05, 0.05)))
    with pytest.raises(ValueError, match="normals must have shape"):
        g.make_mesh(vs, fs, red, normals=want[:-1])
    with pytest.raises(ValueError, match="vertex normal"):
        g.make_mesh(vs, fs, red, normals=bad)
    m = g.make_mesh(vs, fs, red, normals=want)
    assert m.args[-1] is red and len(m.args) == 4 and m.args[2] is None and np.array_equal(m.normals, want)
    assert g.make_mesh(vs, fs, red).normals is None


# ------------------------------------------------------------------ 4. OBJ
def test_read_obj_with_normals(tmp_path):
    p = tmp_path / "a.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvn 0 0 1\nvn 1 0 0\nvn 0 2 0\n"
                 "f 1//1 2//1 3//1\nf 1//2 3//-1 4//2\n")
    vs, fs, uvs, ns = mesh.read_obj(str(p), normals=True)
    # position 1 with two normals becomes two vertices; position 3 with normals 1 and 3 as well
    assert fs.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert vs.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert ns.tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 2, 0], [1, 0, 0]] and uvs is None
    # the default call: its 3-tuple, vertices shared by (v, vt) as before
    vs3, fs3, uvs3 = mesh.read_obj(str(p))
    assert vs3.shape == (4, 3) and fs3.tolist() == [[0, 1, 2], [0, 2, 3]] and uvs3 is None
    q = tmp_path / "b.obj"
    q.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nvn 0 1 1\n"
                 "f 1/1/1 2/2/1 3/3/2 4/4/2\n")
    vs, fs, uvs, ns = mesh.read_obj(str(q), normals=True)
    assert fs.tolist() == [[0, 1, 2], [0, 2, 3]] and vs.shape == (4, 3)
    assert uvs.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] and ns.tolist() == [[0, 0, 1], [0, 0, 1], [0, 1, 1], [0, 1, 1]]
    assert len(mesh.read_obj(str(q))) == 3
    # one corner without vn: no normals (the uvs stay)
    r = tmp_path / "c.obj"
    r.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1\n")
    vs, fs, uvs, ns = mesh.read_obj(str(r), normals=True)
    assert ns is None and uvs is not None and fs.tolist() == [[0, 1, 2]]
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//2\n")
    with pytest.raises(ValueError, match="normal index 2 out of range"):
        mesh.read_obj(str(bad), normals=True)
    mesh.read_obj(str(bad))                                                      # (vn is not looked at by default)
    # a generated smooth mesh written out and read back
    iv, jf = mesh.icosphere(1)
    nn = mesh.radial_normals(iv)
    s = tmp_path / "ball.obj"
    s.write_text("".join("v %r %r %r\n" % tuple(float(x) for x in p3) for p3 in iv) +
                 "".join("vn %r %r %r\n" % tuple(float(x) for x in p3) for p3 in nn) +
                 "".join("f %d//%d %d//%d %d//%d\n" % tuple(int(i) + 1 for i in np.repeat(f, 2)) for f in jf))
    vs, fs, uvs, ns = mesh.read_obj(str(s), normals=True)
    assert np.array_equal(vs[fs], iv[jf]) and np.array_equal(ns[fs], nn[jf]) and vs.shape == iv.shape


# ------------------------------------------------------------------ 5. the ABI's refusals
def test_add_mesh_normals_refuses_bad_normals_without_gpu():
    L = _lib.lib()
    out = ctypes.c_int(-7)
    err = lambda: L.rt_last_error().decode()
    verts = (ctypes.c_double * 12)(0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1)
    faces = (ctypes.c_int32 * 6)(0, 1, 2, 0, 1, 3)
    good = (ctypes.c_double * 12)(0, 0, 1, 0, 0, 2, 0, 1, 1, 1, 0, 0)
    nan = (ctypes.c_double * 12)(0, 0, 1, 0, 0, 2, 0, 1, 1, float("nan"), 0, 0)
    zero = (ctypes.c_double * 12)(0, 0, 1, 0, 0, 2, 0, 0, 0, 1, 0, 0)
    huge = (ctypes.c_double * 12)(0, 0, 1, 0, 0, 2, 0, 1, 1, 1e200, 1e200, 0)
    ref = ctypes.byref(out)
    # refused before the handle is looked at: the handle is no scene's, and the message is about the normal
    assert L.rt_add_mesh_normals(424242, verts, 4, faces, 2, None, nan, 0, ref) != 0
    assert "face 1" in err() and "normal" in err() and "not finite" in err()
    assert L.rt_add_mesh_normals(424242, verts, 4, faces, 2, None, zero, 0, ref) != 0
    assert "face 0" in err() and "normal" in err() and "zero" in err()
    assert L.rt_add_mesh_normals(424242, verts, 4, faces, 2, None, huge, 0, ref) != 0
    assert "face 1" in err() and "non-finite length" in err()
    assert L.rt_add_mesh_normals(424242, verts, 4, faces, 2, None, good, 0, None) != 0 and "null" in err()
    assert L.rt_add_mesh_normals(424242, verts, 4, (ctypes.c_int32 * 6)(0, 1, 2, 0, 1, 4), 2, None, good, 0, ref) != 0
    assert "face 1" in err() and "out of range" in err()
    # good normals, and none at all, get as far as the handle
    assert L.rt_add_mesh_normals(424242, verts, 4, faces, 2, None, good, 0, ref) != 0 and "invalid scene handle" in err()
    assert L.rt_add_mesh_normals(424242, verts, 4, faces, 2, None, None, 0, ref) != 0 and "invalid scene handle" in err()
    assert L.rt_add_mesh(424242, verts, 4, faces, 2, None, 0, ref) != 0 and "invalid scene handle" in err()
    assert out.value == -7                                                       # no refusal wrote the result


def test_abi_announces_smooth_normals():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt) and re.search(r"#define\s+RT_HAS_SMOOTH_NORMALS\s+1\b", txt)
    assert "rt_add_mesh_normals" in _lib.EXPORTED and "rt_add_mesh" in _lib.EXPORTED
    assert "There are no per-vertex shading normals" not in txt
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rt_add_mesh_normals" in doc and "RT_HAS_SMOOTH_NORMALS" in doc
    sc = scenes.SCENES["cornell_smooth"](16, 16)
    ball = sc.obj_list[-1]
    assert ball.kind == "mesh" and ball.args[1].shape == (1280, 3) and ball.normals.shape == ball.args[0].shape
    assert ball.args[-1].kind == "metal"


# ------------------------------------------------------------------ 6. the build under sanitizers
@pytest.fixture(scope="module")
def smooth_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("smooth") / "smooth_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "csrc", "smooth_check.cpp"), os.path.join(CSRC, "rt_build.cpp")])
    return exe


def test_scene_build_with_vertex_normals_under_sanitizers(smooth_check):
    """Two 80-triangle meshes with distinct normals (no chain; rotate-y + translate) and a plain one: every TriNrm
    belongs to the triangle of the TriRec at its index, has = 0 on the plain mesh, tri_smooth set, 1 and 8
    threads one digest; no sanitizer report."""
    r = subprocess.run([smooth_check], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip()[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout)
    assert res["ok"] and res["error"] == ""
    assert res["n_tri"] == 240 and res["n_nrm"] == 240 and res["smooth"] == 160 and res["plain"] == 80
    assert res["unknown"] == 0 and res["mismatched"] == 0 and res["plain_bad"] == 0 and res["not_unit"] == 0
    assert res["tri_smooth"] == 1 and res["same_threads"]
    assert res["flat_ok"] and res["flat_tri_smooth"] == 0 and res["flat_plain"] == 80 and res["flat_bad"] == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr.strip() == ""


# ------------------------------------------------------------------ 7. the scatter helper
def _oracle_scene(oracle_mod, material):
    """Spheres and rects of one material, seen from all sides."""
    objs = [g.make_sphere(v.vec3(0, 0, 0), 2.0, material), g.make_sphere(v.vec3(5, 0.5, -1), 1.0, material),
            g.make_xz_rect(-8, 8, -8, 8, -2.5, material), g.flip_normals(g.make_xy_rect(-8, 8, -3, 6, -6, material)),
            g.make_yz_rect(-3, 6, -8, 8, -7.5, material)]
    cam = make_camera(v.vec3(0, 3, 12), v.vec3(0, 0, 0), v.vec3(0, 1, 0), 40, 1.0, 0, 1, 0, 1)
    return oracle_mod.build_scene(g.make_scene(objs, cam, g.sky_color))


def _records(n, seed):
    rng = np.random.RandomState(seed)
    o = rng.uniform(-6, 6, (n, 3))
    o[n // 4:, 1] = np.abs(o[n // 4:, 1]) + 1.0
    o[:n // 4] = rng.normal(size=(n // 4, 3)) * 0.4                                # inside the big sphere: dot(d, n) > 0
    tgt = rng.uniform(-3, 3, (n, 3))
    tgt[: n // 4] = rng.normal(size=(n // 4, 3)) * 5.0
    d = (tgt - o) * rng.uniform(0.2, 3.0, (n, 1))
    return np.concatenate([o, d, np.zeros((n, 1))], axis=1)


@pytest.mark.parametrize("name,material", [
    ("metal fuzz 0", g.make_metal(g.constant_texture((0.7, 0.6, 0.5)), 0.0)),
    ("metal fuzz 0.3", g.make_metal(g.constant_texture((0.8, 0.85, 0.88)), 0.3)),
    ("dielectric 1.5", g.make_dielectric(1.5)),
])
def test_scatter_helper_reproduces_the_oracle(oracle_mod, name, material):
    """smooth_cases.scatter fed orc_step's own hit point and normal: STEP_D, STEP_A, the survival, the origin and
    the draw counter bit for bit, at depth 1 with varied start counters."""
    import oracle
    osc = _oracle_scene(oracle_mod, material)
    rays = _records(900, 11)
    ctr_in = (np.arange(len(rays)) * 7 % 41).astype(np.uint32)
    rows, ctr = osc.step(rays, 1, sm.SEED, sm.SMP, ctr_in=ctr_in)
    hit = rows[:, oracle.STEP_HIT] == 1
    assert hit.sum() >= 500
    survived = absorbed = inside = 0
    for k in np.nonzero(hit)[0]:
        ok, o, d, a, c = sm.scatter(rows[k, oracle.STEP_P], rows[k, oracle.STEP_N], rays[k], material, sm.SEED, int(k), sm.SMP,
                                    int(ctr_in[k]))
        assert ok == (rows[k, oracle.STEP_KIND] == 1), (name, k)
        assert c == int(ctr[k]), (name, k, c, ctr[k])
        inside += float(np.dot(rays[k, 3:6], rows[k, oracle.STEP_N])) > 0
        if not ok:
            absorbed += 1
            continue
        survived += 1
        for got, col in ((d, oracle.STEP_D), (a, oracle.STEP_A), (o, oracle.STEP_O)):
            assert np.array_equal(np.array(got).view(np.uint64), rows[k, col].view(np.uint64)), (name, k, got, rows[k, col])
    print("%s: %d records, %d survive, %d absorbed, %d from the inside" % (name, hit.sum(), survived, absorbed, inside))
    assert survived >= 300 and inside >= 50
    if material.kind == "metal":
        assert absorbed >= 20                                                     # (reflections off the back: below the normal)
    # the depth cap ends the path in the helper as in the oracle
    rows, ctr = osc.step(rays[hit][:20], sm.KMAX, sm.SEED, sm.SMP)
    for k in range(len(rows)):
        ok, _, _, _, c = sm.scatter(rows[k, oracle.STEP_P], rows[k, oracle.STEP_N], rays[hit][k], material, sm.SEED, k, sm.SMP, 0,
                                    depth=sm.KMAX)
        assert not ok and rows[k, oracle.STEP_KIND] == 0 and c == int(ctr[k])
