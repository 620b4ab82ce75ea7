"""Light lists on the GPU (RT_HAS_LIGHT_LIST), on the scenes, points and directions of tests/light_cases.py.

The truth for the sampler and the density is rtamd.lights (the NumPy restatement of include/rt.h's "light
lists", itself pinned to the oracle in test_light_list_host.py): rt_light_probe equals it bit for bit.  Renders
are compared with the single-light renders they must equal, with themselves under other schedules, and
statistically with cornell_mixture, whose lamp the lists restate."""
import ctypes

import numpy as np
import pytest

import light_cases as lc
from rtamd import _lib, gpu, lights, mesh, scenes
from rtamd import scene as g

pytestmark = pytest.mark.gpu

NX, NY, SEED = lc.NX, lc.NY, lc.SEED


def _render(scene, first, passes, seed=SEED):
    acc = np.zeros(NX * NY * 3)
    h = gpu.render_host(scene, NX, NY, first, passes, seed, acc)
    return acc, gpu.stats(h)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# --------------------------------------------------- 1. the probe equals the restatement
@pytest.mark.parametrize("name", list(lc.PROBE_LISTS))
def test_probe_equals_the_restatement(sched, name):
    sc = lc.probe_scene(name)
    pts, dirs = lc.probe_points(name)
    lst = lights.flatten(sc.lights)
    want = [lights.random(lst, pts[k], SEED, k) for k in range(len(pts))]
    want_dir = np.array([w[0] for w in want])
    want_draws = np.array([w[1] for w in want], dtype=np.int32)
    with np.errstate(all="ignore"):
        want_pdf, want_pdf_dirs = lights.pdf_value(lst, pts, want_dir), lights.pdf_value(lst, pts, dirs)
    hits = int((want_pdf_dirs > 0).sum())
    print("%s: %d lights, %d points; dirs: %d with a positive density, %d NaN; sampled dirs: %d positive"
          % (name, len(lst), len(pts), hits, int(np.isnan(want_pdf_dirs).sum()), int((want_pdf > 0).sum())))
    assert hits > len(pts) // 8 and (want_pdf_dirs == 0).sum() > len(pts) // 16    # (the cases are not all of one kind)
    for mode in (("exact",) if name in lc.HAS_SPHERE else ("exact", "device")):
        sched.set_option("exact_libm", mode)
        got_dir, got_pdf, got_pdf_dirs, got_draws = gpu.light_probe(sc, pts, SEED, dirs)
        bad = {"out_dir": int((~_same_bits(got_dir, want_dir)).any(axis=1).sum()),
               "out_pdf": int((~_same_bits(got_pdf, want_pdf)).sum()),
               "out_pdf_dirs": int((~_same_bits(got_pdf_dirs, want_pdf_dirs)).sum()),
               "out_draws": int((got_draws != want_draws).sum())}
        print("%s, libm %s: differing %r" % (name, mode, bad))
        assert not any(bad.values()), (mode, bad)
        # without dirs: the same first three outputs
        d2, p2, none, n2 = gpu.light_probe(sc, pts, SEED)
        assert none is None and np.array_equal(n2, got_draws) and _same_bits(d2, got_dir).all() and _same_bits(p2, got_pdf).all()


def test_shared_edge_counts_both_triangles(sched):
    """A direction at the quad's shared diagonal or a vertex of it hits both triangles: the list's density there is
    the sum of two equal halves, on the device as in NumPy."""
    sc = lc.probe_scene("two_tris")
    t0, t1 = [L[1] for L in lights.flatten(sc.lights)]
    shared = [v for v in t0 if any((v == w).all() for w in t1)]
    assert len(shared) == 2
    o = np.array([278.0, 100.0, 278.0])
    targets = np.array([shared[0], shared[1], 0.5 * (shared[0] + shared[1]), 0.25 * shared[0] + 0.75 * shared[1]])
    pts = np.repeat(o[None], len(targets), axis=0)
    dirs = targets - o
    one = np.array([lights.pdf_value([L], o, dirs) for L in lights.flatten(sc.lights)])
    _, _, got, _ = gpu.light_probe(sc, pts, SEED, dirs)
    want = lights.pdf_value(sc.lights, o, dirs)
    print("shared edge: per-triangle densities", one.tolist(), "list", got.tolist())
    assert _same_bits(got, want).all()
    assert ((one[0] > 0) & (one[1] > 0)).sum() >= 2              # the exact vertices at least count twice


# ------------------------------------------------------- 2. a list of one is the light
@pytest.mark.parametrize("which", ["cornell_mixture", "sphere_light"])
def test_list_of_one_is_the_light(sched, which):
    if which == "cornell_mixture":
        single, as_list = scenes.cornell_mixture(NX, NY), lc.room(lights=[scenes.cornell_box(NX, NY).obj_list[2]])
    else:
        single, as_list = lc.sphere_scene(), lc.sphere_scene(lights=True)
    a, sa = _render(single, 0, 16)
    b, sb = _render(as_list, 0, 16)
    print("%s: segments %d / %d" % (which, sa.segments, sb.segments))
    assert np.isfinite(a).all() and a.sum() > 0
    assert np.array_equal(a, b) and sa.segments == sb.segments


# ----------------------------------------------------------- 3. schedule invariance
@pytest.mark.parametrize("which", ["two_triangle_lamp", "cornell_mesh_lights"])
def test_render_is_schedule_invariant(sched, which):
    sc = lc.room(lights=lc.lamp_triangles()) if which == "two_triangle_lamp" else scenes.SCENES["cornell_mesh_lights"](NX, NY)
    base, st = _render(sc, 0, 16)
    assert np.isfinite(base).all() and base.sum() > 0 and st.segments > st.paths
    if which == "cornell_mesh_lights":                               # its own lamp is sampled: not cornell_mesh's image
        assert not np.array_equal(base, _render(scenes.SCENES["cornell_mesh"](NX, NY), 0, 16)[0])
    sched.set_option("tail_off", 1)
    assert np.array_equal(_render(sc, 0, 16)[0], base)
    sched.reset_options()
    sched.set_option("lanes", 1)
    one, st1 = _render(sc, 0, 16)
    sched.set_option("lanes", 2)
    sched.set_option("max_paths", 4096)
    two, st2 = _render(sc, 0, 16)
    print("lanes/chunks:", st1.lanes, st1.chunks, st2.lanes, st2.chunks, "finish paths", st.finish_paths)
    assert st1.lanes == 1 and st2.lanes == 2 and st2.chunks > 2
    assert np.array_equal(one, base) and np.array_equal(two, base)


# ------------------------------------------- 4. the render agrees with the pinned estimator
def test_lists_render_like_the_single_light(sched):
    """cornell_mixture (seed S) against the same room with the lamp as two half rects (S + 1) and as two
    triangles (S + 2): the lists sample the same points with the same density, so the clamped per-sample
    statistic A = mean over channels of min(x, 1) has one law.  64 passes, one at a time; the frame means differ
    by at most 5 combined standard errors."""
    passes = 64
    cases = [("cornell_mixture", lc.room(light="own"), SEED), ("two half rects", lc.room(lights=lc.lamp_halves()), SEED + 1),
             ("two triangles", lc.room(lights=lc.lamp_triangles()), SEED + 2)]
    stats = []
    for name, sc, seed in cases:
        S, Q = lc.clamped_moments(lambda k: _render(sc, k, 1, seed)[0], passes)
        m, var = lc.mean_and_var(S, Q, passes)
        print("%-16s frame mean of A %.6f, se %.3e" % (name, m, np.sqrt(var)))
        stats.append((m, var))
    (ma, va) = stats[0]
    assert ma > 0.1
    for (name, _, _), (mb, vb) in zip(cases[1:], stats[1:]):
        se = float(np.sqrt(va + vb))
        print("%-16s |difference| %.3e = %.2f combined standard errors" % (name, abs(ma - mb), abs(ma - mb) / se))
        assert abs(ma - mb) <= 5.0 * se, (name, ma, mb, se)


# ------------------------------------------------------------------ 5. ABI refusals
def test_abi_refusals_and_last_call_wins(sched):
    L = _lib.lib()
    err = lambda: L.rt_last_error().decode()
    b = gpu.GpuBuilder(sched)
    s = b.scene
    lam = b.material_lambertian(b.texture_constant((0.5, 0.5, 0.5)))
    sph, rect = b.sphere((0, 1, 0), 1, lam), b.rect(1, -1, 1, -1, 1, 3, lam)
    tri = b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), lam)
    ints = lambda *v: (ctypes.c_int * max(1, len(v)))(*v)
    refused = {"box": b.box((0, 0, 0), (1, 1, 1), lam), "moving sphere": b.moving_sphere((0, 0, 0), (0, 1, 0), 0, 1, 1, lam),
               "translate": b.translate(sph, (1, 0, 0)), "rotate-y": b.rotate_y(rect, 10.0), "bvh": b.bvh([sph, rect], 0, 1, 0),
               "curve": b.bezier((0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 1, 0), 0.1, lam),
               "medium": b.constant_medium(sph, 0.5, b.texture_constant((1, 1, 1))), "klein": b.klein((0, 0, 0), lam)}
    b.set_lights([sph])                                              # the setting every refusal must leave alone
    for name, obj in refused.items():
        for lst in ((obj,), (rect, b.list([tri, b.list([obj])]))):
            assert L.rt_set_light_list(s, ints(*lst), len(lst)) != 0, name
            assert "a light must be a rect, a sphere or a triangle" in err(), (name, err())
    assert L.rt_set_light_list(s, ints(sph, 10 ** 6), 2) != 0 and "invalid object id" in err()
    assert L.rt_set_light_list(s, ints(-3), 1) != 0 and "invalid object id" in err()
    assert L.rt_set_light_list(s, ints(b.list([b.list([])])), 1) != 0 and "holds no light" in err()
    assert L.rt_set_light_list(s, None, 2) != 0 and "null" in err()
    assert L.rt_set_light_list(s, ints(sph), -1) != 0 and ">= 0" in err()
    vs, fs = mesh.icosphere(3)                                       # 1280 faces: four of them pass the cap
    big = [b.mesh(vs, fs, None, lam) for _ in range(4)]
    assert L.rt_set_light_list(s, ints(*big[:3], b.list([tri] * 256)), 4) == 0          # 4096 exactly
    assert L.rt_set_light_list(s, ints(*big[:3], b.list([tri] * 257)), 4) != 0 and "RT_MAX_LIGHTS" in err()
    one_mesh = np.concatenate([vs[fs].reshape(-1, 3)] * 4)[: 4097 * 3]
    m4097 = b.mesh(one_mesh, np.arange(4097 * 3, dtype=np.int32).reshape(-1, 3), None, lam)
    assert L.rt_set_light_list(s, ints(m4097), 1) != 0 and "RT_MAX_LIGHTS" in err()
    assert L.rt_set_light_list(424242, ints(sph), 1) != 0 and "invalid scene handle" in err()
    # last call wins: list -> single -> list -> off, read back through the probe's draws after the commit
    b.set_lights([sph, rect, tri])
    b.set_light(rect)
    b.set_camera(lc.probe_scene("rect").camera.slots())
    world = b.list([sph, rect, tri])
    h = b.commit(world)
    pts = np.array([[0.2, 0.1, 0.3], [0.5, 0.2, -0.4]])
    out_dir, out_pdf, draws = np.zeros((2, 3)), np.zeros(2), np.zeros(2, dtype=np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    args = (pts.ctypes.data_as(dp), None, ctypes.c_uint64(SEED), out_dir.ctypes.data_as(dp), out_pdf.ctypes.data_as(dp), None,
            draws.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert L.rt_light_probe(h, 2, *args) == 0, err()
    assert draws.tolist() == [2, 2] and np.allclose(out_dir[:, 1] + pts[:, 1], 3.0)   # the rect alone: no choice draw
    assert L.rt_light_probe(h, -1, *args) != 0 and ">= 0" in err()
    assert L.rt_light_probe(h, 2, None, *args[1:]) != 0 and "null" in err()
    assert L.rt_light_probe(h, 2, args[0], pts.ctypes.data_as(dp), *args[2:]) != 0 and "null together" in err()
    assert L.rt_set_light_list(h, ints(sph), 1) != 0 and "already committed" in err()
    assert L.rt_set_light_sampling(h, sph) != 0 and "already committed" in err()
    # the other order, and off: rt_set_light_sampling, then the list wins; n == 0 turns sampling off
    for final, want in (("list", [3, 3]), ("off", None)):
        b2 = gpu.GpuBuilder(sched)
        lam2 = b2.material_lambertian(b2.texture_constant((0.5, 0.5, 0.5)))
        r2, t2 = b2.rect(1, -1, 1, -1, 1, 3, lam2), b2.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), lam2)
        b2.set_light(r2)
        b2.set_lights([r2, t2] if final == "list" else [])
        b2.set_camera(lc.probe_scene("rect").camera.slots())
        h2 = b2.commit(b2.list([r2, t2]))
        rc = L.rt_light_probe(h2, 2, *args)
        if want is None:
            assert rc != 0 and "no light sampling" in err()
        else:
            assert rc == 0 and draws.tolist() == want, (rc, err(), draws)
        _lib.call("rt_scene_destroy", h2)
    _lib.call("rt_scene_destroy", h)


def test_python_scene_with_lights_probe_refuses_without(sched):
    with pytest.raises(_lib.RtError, match="no light sampling"):
        gpu.light_probe(scenes.cornell_box(NX, NY), np.zeros((1, 3)), SEED)
