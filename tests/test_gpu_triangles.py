"""Triangles and triangle meshes on the GPU (RT_HAS_TRIANGLES), on the scenes and rays of tests/mesh_cases.py.

The truth for closest hits is rtamd.mesh (the NumPy restatement of include/rt.h's "triangles") merged with the
oracle's flat list for the leaves the oracle can hold: t and material bit for bit.  Renders are compared with
the oracle's render of the same room in rects (cornell_lifted) under the project's own parity gate, with
themselves under other schedules bit for bit, and statistically with an analytic sphere."""
import functools

import numpy as np
import pytest
import torch

import feature_cases as fc
import hit_ray_cases as hc
import mesh_cases as mc
from conftest import host_threads
from rtamd import denoise, gpu, mesh, scenes
from rtamd import scene as g
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

SEED = 0x5EED0602
NX = NY = 48


def _compare(a, b, n):
    d = np.abs(a / n - b / n)
    px = d.reshape(-1, 3).max(axis=1)
    return float(np.sqrt(np.mean(d ** 2))), float(d.max()), int((px > 1e-9).sum()), px.size


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


@functools.lru_cache(maxsize=None)
def _cornell(name):
    return scenes.SCENES[name](NX, NY)


def _render(scene, passes, seed=SEED):
    acc = np.zeros(NX * NY * 3)
    h = gpu.render_host(scene, NX, NY, 0, passes, seed, acc)
    return acc, gpu.stats(h)


# ------------------------------------------------------------------ 1. hit probes
@pytest.mark.parametrize("name", list(mc.SCENES))
def test_hit_probes_equal_the_restatement(sched, oracle_mod, name):
    """rt_hit_rays and rt_hit_rays_stream on every ray class: t the same double, hit / miss and material equal."""
    sc = mc.scene_of(name)
    classes, rays, cls = mc.scene_rays(name)
    want_t, want_m = mc.expected(oracle_mod, name)
    ti, si = gpu.tree_info(gpu.upload(sc)), gpu.scene_info(gpu.upload(sc))
    print(name, ti)
    assert ti["tri_leaves"] == mc.TRI_LEAVES[name] and ti["group_leaves"] == 0
    assert si["extend_lds_bytes"] == 0 and si["camera_lds_bytes"] == 0
    for walk in (hc.WALK_LDS_TIME0, hc.WALK_LDS_CAMERA):
        with pytest.raises(RtError, match="LDS"):
            gpu.hit_rays(sc, rays[:1], walk=walk)
    t, m = gpu.hit_rays(sc, rays)
    ts, ms, draws = gpu.hit_rays_stream(sc, rays, SEED)
    bad = []
    for i, c in enumerate(classes):
        sel = cls == i
        hits = int((want_m[sel] >= 0).sum())
        nbad = int((~hc.same_t(t[sel], want_t[sel]) | (m[sel] != want_m[sel])).sum())
        nbad_s = int((~hc.same_t(ts[sel], want_t[sel]) | (ms[sel] != want_m[sel])).sum())
        print("%s %-16s rays %5d hits %5d differing: rt_hit_rays %d, rt_hit_rays_stream %d" % (name, c, sel.sum(), hits, nbad, nbad_s))
        if nbad or nbad_s:
            bad.append((c, nbad, nbad_s))
    assert not bad, bad
    assert (draws == 0).all()
    by = dict(zip(classes, range(len(classes))))
    if name in ("quad", "coincident_triangles"):                   # in the plane z = -1 exactly: a miss
        assert (want_m[cls == by["in_plane"]] >= 0).sum() == 0
    # (a ray aimed at the open border of a lone triangle may round to either side: only some must hit)
    assert (want_m[cls == by["edges_vertices"]] >= 0).sum() > 20 and (want_m[cls == by["random"]] >= 0).sum() > 200
    k = cls == by["tmin"]
    assert (want_m[k] >= 0).sum() > 0
    if name in ("one_triangle", "quad", "coincident_triangles", "instanced_quad"):   # triangles only, and open
        assert (want_m[cls == by["nonfinite"]] >= 0).sum() == 0    # (a rect takes a NaN t, Q20)
        assert (want_m[k] >= 0).sum() < k.sum()                    # t = 0.001 lies between the origins


def test_list_order_decides_ties(sched, oracle_mod):
    """Coincident triangles: the first in list order; a triangle coincident with a rect: the rect, in both orders."""
    ray = np.array([[0.5, -0.5, 3.0, 0.0, 0.0, -1.0, 0.0]])
    for name, want in (("coincident_triangles", 0), ("rect_then_triangles", 0), ("triangles_then_rect", 1)):
        t, m = gpu.hit_rays(mc.scene_of(name), ray)
        assert t[0] == 4.0 and m[0] == want, (name, t, m)


def test_flip_normals_negates_the_triangle_normal(sched):
    """instanced_quad (flip + rotate-y + translate): the feature buffers' normal is the geometric one negated and
    taken out of the chain, exactly, on every pixel whose one camera sample hits."""
    sc = mc.scene_of("instanced_quad")
    lf = mc.leaves_of(sc)[0]
    assert lf.flip and len(lf.ops) == 2
    want = mesh.out_of_instance(-mesh.normal(lf.tris), lf.ops)     # (the flip comes before the chain, as on the device)
    assert np.array_equal(want[0], want[1])                        # a planar quad: one normal
    feat = np.zeros(NX * NY * 8)
    gpu.render_features_host(sc, NX, NY, 0, 1, SEED, feat)
    f = feat.reshape(-1, 8)
    hit = f[:, 7] == 1.0
    print("flipped quad: %d of %d pixels hit, normal %r" % (hit.sum(), hit.size, want[0].tolist()))
    assert hit.sum() > 100 and (~hit).sum() > 100
    assert (f[hit, 3:6] == want[0]).all()                          # (exact; a sum from 0 turns the -0 of y into +0)
    assert (f[~hit, 3:6] == 0.0).all()
    # the same quad without the flip: the opposite normal
    vs, fs, uvs = mesh.quad(*mc.QUAD)
    plain = g.make_scene([g.translate(g.rotate_y(g.make_mesh(vs, fs, lf.material, uvs), 37.0), (0.5, 0.25, -1.0))],
                         mc._cam(), g.sky_color)
    feat2 = np.zeros(NX * NY * 8)
    gpu.render_features_host(plain, NX, NY, 0, 1, SEED, feat2)
    assert np.array_equal(feat2.reshape(-1, 8)[hit, 3:6], -f[hit, 3:6])


# ------------------------------------------------------------- 2. watertightness
def test_watertight_on_the_device(sched):
    rays, vs, fs = mc.watertight_rays()
    white = g.make_lambertian(g.constant_texture((0.7, 0.7, 0.7)))
    sc = g.make_scene([g.make_mesh(vs, fs, white)], mc._cam(), g.sky_color)
    t, m = gpu.hit_rays(sc, rays)
    want_t, want_i = mesh.hit(vs[fs], rays)
    print("watertight on the device: %d rays, %d missed" % (len(rays), int((m < 0).sum())))
    assert int((m < 0).sum()) == 0
    assert hc.same_t(t, want_t).all()


# ------------------------------------------------------------------- 3. features
@functools.lru_cache(maxsize=None)
def _mesh_features(passes):
    """cornell_mesh's expected features: the oracle's camera rays (trace_sample on cornell_lifted; the camera
    ray does not depend on the objects), first hits, normals and albedo from rtamd.mesh."""
    import oracle
    o = oracle.build_scene(_cornell("cornell_lifted"))
    npx = NX * NY
    rays = np.zeros((npx * passes, 7))
    sky = np.zeros((npx * passes, 3))
    for j in range(npx):
        y, x = divmod(j, NX)
        for smp in range(passes):
            row = o.trace_sample(NX, NY, x, y, SEED, smp, cap=1)[0]
            rays[j * passes + smp, 0:6] = row[0:6]
            sky[j * passes + smp] = fc.sky_gradient(row[3:6])
    n = len(rays)
    t = np.full(n, mesh.TMAX)
    alb, nrm = sky.copy(), np.zeros((n, 3))
    hit = np.zeros(n)
    for lf in mc.leaves_of(_cornell("cornell_mesh")):
        tt, idx = mesh.hit(lf.tris, mesh.into_instance(rays, lf.ops))
        take = (idx >= 0) & (tt < t)
        t = np.where(take, tt, t)
        normals = mesh.out_of_instance(mesh.normal(lf.tris), lf.ops)
        nrm[take] = normals[idx[take]]
        alb[take] = np.array(lf.material.args[0].args[0])
        hit[take] = 1.0
    per = np.concatenate([alb, nrm, np.where(hit > 0, t, 0.0)[:, None], hit[:, None]], axis=1).reshape(npx, passes, 8)
    feat = np.zeros((npx, 8))
    for smp in range(passes):
        feat = feat + per[:, smp]
    return feat


def test_features_of_cornell_mesh(sched):
    passes = fc.FEATURE_PASSES
    want = _mesh_features(passes)
    feat = np.zeros(NX * NY * 8)
    gpu.render_features_host(_cornell("cornell_mesh"), NX, NY, 0, passes, SEED, feat)
    got = feat.reshape(-1, 8)
    diff = got.view(np.uint64) != want.view(np.uint64)
    print("cornell_mesh features: %d of %d values differ; hit samples %d of %d" % (diff.sum(), diff.size, int(want[:, 7].sum()), NX * NY * passes))
    assert want[:, 7].sum() > 0.5 * NX * NY * passes
    assert not diff.any(), np.argwhere(diff)[:8]


# -------------------------------------------------------- 4. schedule invariance
def test_render_is_schedule_invariant(sched):
    sc = _cornell("cornell_mesh")
    base, st = _render(sc, 16)
    assert np.isfinite(base).all() and base.sum() > 0 and st.segments > st.paths
    sched.set_option("tail_off", 1)
    assert np.array_equal(_render(sc, 16)[0], base)
    sched.reset_options()
    sched.set_option("lanes", 1)
    one, st1 = _render(sc, 16)
    sched.set_option("lanes", 2)
    sched.set_option("max_paths", 4096)
    two, st2 = _render(sc, 16)
    print("lanes/chunks:", st1.lanes, st1.chunks, st2.lanes, st2.chunks, "finish paths", st.finish_paths)
    assert st1.lanes == 1 and st2.lanes == 2 and st2.chunks > 2
    assert np.array_equal(one, base) and np.array_equal(two, base)


# ---------------------------------------------------------------- 5. path parity
def test_path_parity_with_the_oracle_on_the_room_in_rects(sched, oracle_mod):
    """cornell_mesh on the GPU against the oracle's cornell_lifted, 48x48x16, RT_LIBM_EXACT: the two differ by a
    few ulps of t per segment; the project's gate (test_horizon_rows_exact_libm): at most 0.5 % of the pixels
    off by more than 1e-9 in the mean."""
    n = 16
    sched.set_option("exact_libm", "exact")
    acc, st = _render(_cornell("cornell_mesh"), n)
    ref, segs = oracle_mod.build_scene(_cornell("cornell_lifted")).render(NX, NY, 0, n, SEED, nthreads=host_threads())
    rms, dmax, nbad, npx = _compare(acc, ref, n)
    print("cornell_mesh vs the oracle's cornell_lifted: rms=%.3e max=%.3e pixels>1e-9: %d/%d; segments gpu %d oracle %d"
          % (rms, dmax, nbad, npx, st.segments, segs))
    assert nbad <= npx // 200, (rms, dmax, nbad, npx)


# ------------------------------------------------------ 6. a curved mesh, statistically
def _room_with(ball):
    room = [o for o in _cornell("cornell_lifted").obj_list[:6]]
    return g.make_scene(room + [ball], scenes.cornell_camera_for(NX, NY), g.sky_color)


def _moments(sc, passes):
    npx = NX * NY
    S, Q = _dev(np.zeros(npx * 3)), _dev(np.zeros(npx * 3))
    cnt = _dev(np.zeros(npx, dtype=np.uint32))
    pix = _dev(gpu.shard_pixels(NX, NY, 0, 1))
    gpu.render_pixels_device(sc, NX, NY, pix.data_ptr(), npx, 0, passes, SEED, S.data_ptr(), Q.data_ptr(), cnt.data_ptr())
    feat = _dev(np.zeros(npx * 8))
    gpu.render_features_device(sc, NX, NY, 0, passes, SEED, feat.data_ptr())
    torch.cuda.synchronize()
    return (S.cpu().numpy().reshape(-1, 3), Q.cpu().numpy().reshape(-1, 3), cnt.cpu().numpy().view(np.uint32),
            feat.cpu().numpy().reshape(-1, 8))


def test_icosphere_lights_the_room_like_the_sphere(sched):
    """icosphere(3) against the analytic sphere of its radius: over the pixels whose camera samples all hit
    the same wall / floor materials in both scenes, the mean radiance differs by at most 5 combined standard
    errors (from accum2); the seed is fixed."""
    passes, c, r = 64, (278.0, 120.0, 278.0), 90.0
    grey = g.make_lambertian(g.constant_texture((0.5, 0.5, 0.5)))
    vs, fs = mesh.icosphere(3, radius=r, center=c)
    Sa, Qa, ca, fa = _moments(_room_with(g.make_mesh(vs, fs, grey)), passes)
    Sb, Qb, cb, fb = _moments(_room_with(g.make_sphere(c, r, grey)), passes)
    assert (ca == passes).all() and (cb == passes).all()
    ball = np.zeros(3)
    for _ in range(passes):
        ball = ball + 0.5
    around = (fa[:, 7] == passes) & (fb[:, 7] == passes) & (fa[:, 0:3] == fb[:, 0:3]).all(axis=1) & \
        (fa[:, 0:3] != ball).any(axis=1)
    on_ball = (fa[:, 0:3] == ball).all(axis=1)
    assert around.sum() > 500 and on_ball.sum() > 50, (around.sum(), on_ball.sum())

    def mean_and_var(S, Q):
        m = S[around] / passes
        var_mean = (Q[around] / passes - m * m) * (passes / (passes - 1.0)) / passes
        return m.mean(), var_mean.sum() / m.size ** 2
    ma, va = mean_and_var(Sa, Qa)
    mb, vb = mean_and_var(Sb, Qb)
    se = float(np.sqrt(va + vb))
    print("icosphere(3) vs sphere: %d pixels around the ball, mean radiance %.6f / %.6f, difference %.3e = %.2f combined "
          "standard errors (%.3e)" % (around.sum(), ma, mb, abs(ma - mb), abs(ma - mb) / se, se))
    assert abs(ma - mb) <= 5.0 * se


# ----------------------------------------------------------- 7. image-textured mesh
def test_image_textured_quad_equals_the_rect(sched):
    """A quad with uvs (0,0) (1,0) (1,1) (0,1) and a 5x3 image against the same rect with the same image: the
    albedo of every camera sample bit for bit, but for at most 0.5 % of the samples, which fall on the
    neighbouring texel where the two u, v formulas round apart on a texel boundary."""
    rng = np.random.RandomState(5)
    data = rng.randint(0, 256, 5 * 3 * 3).astype(np.uint8)
    vs, fs, uvs = mesh.quad(*mc.QUAD)
    scenes_ = []
    for as_mesh in (True, False):
        m = g.make_lambertian(g.make_image_texture(data, 5, 3))
        obj = g.make_mesh(vs, fs, m, uvs) if as_mesh else g.make_xy_rect(-1.0, 1.0, -1.0, 1.0, -1.0, m)
        scenes_.append(g.make_scene([obj], mc._cam(), g.sky_color))
    differ = total = 0
    for smp in range(4):
        f = [np.zeros(NX * NY * 8), np.zeros(NX * NY * 8)]
        for k in (0, 1):
            gpu.render_features_host(scenes_[k], NX, NY, smp, 1, SEED, f[k])
        a, b = f[0].reshape(-1, 8), f[1].reshape(-1, 8)
        assert np.array_equal(a[:, 7], b[:, 7]) and np.array_equal(a[:, 3:6], b[:, 3:6])
        hit = a[:, 7] == 1.0
        total += int(hit.sum())
        differ += int((a[hit, 0:3] != b[hit, 0:3]).any(axis=1).sum())
        texels = {tuple(data[3 * i:3 * i + 3] / 255.0) for i in range(15)}
        assert all(tuple(x) in texels for x in a[hit, 0:3])
    print("image-textured quad vs rect: %d of %d samples on another texel" % (differ, total))
    assert total > 1000 and differ <= total // 200


# ------------------------------------------------------- 8. adaptive render, denoiser
def test_adaptive_render_is_the_uniform_render_of_each_count(sched):
    sc = _cornell("cornell_mesh")
    lo, hi, step = 4, 16, 4
    acc, acc2, cnt, res = gpu.render_adaptive_host(sc, NX, NY, gpu.adaptive_params(0.05, lo, hi, step), SEED)
    acc, acc2 = acc.reshape(-1, 3), acc2.reshape(-1, 3)
    S, Q = np.zeros((NX * NY, 3)), np.zeros((NX * NY, 3))
    for k in range(hi):
        p = np.zeros(NX * NY * 3)
        gpu.render_host(sc, NX, NY, k, 1, SEED, p)
        p = p.reshape(-1, 3)
        on = (cnt > k)[:, None]
        S = np.where(on, S + p, S)
        Q = np.where(on, Q + p * p, Q)
    print("adaptive on cornell_mesh:", res, np.bincount(cnt)[lo::step])
    assert set(np.unique(cnt)) <= set(range(lo, hi + 1, step)) and len(np.unique(cnt)) > 1
    assert np.array_equal(acc, S) and np.array_equal(acc2, Q)


def test_denoise_runs_on_a_mesh_scene(sched):
    passes = 16
    S, Q, cnt, feat = _moments(_cornell("cornell_mesh"), passes)
    want = denoise.atrous(S.ravel(), Q.ravel(), cnt, 0, feat.ravel(), passes, NX, NY)
    d_s, d_q, d_c, d_f = _dev(S.ravel()), _dev(Q.ravel()), _dev(cnt), _dev(feat.ravel())
    d_o = _dev(np.full(NX * NY * 3, -3.0))
    gpu.denoise_device(NX, NY, gpu.denoise_params(), d_s.data_ptr(), d_q.data_ptr(), d_c.data_ptr(), 0, d_f.data_ptr(),
                       passes, d_o.data_ptr())
    got = d_o.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print("denoise on cornell_mesh: max |device - numpy| = %.3e = %.3e * max |out|" % (err, err / scale))
    assert err <= 1e-12 * scale                                    # (test_gpu_denoise's bound)
    assert np.abs(want - S.ravel() / passes).max() > 1e-3          # the filter did something


# ------------------------------------------------------------- 9. commit refusals
def test_commit_refuses_what_the_header_says(sched):
    red = g.make_lambertian(g.constant_texture((0.65, 0.05, 0.05)))
    tri = g.make_triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), red)
    cam = mc._cam()
    curve = g.make_bezier((0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 1, 0), 0.1, red)
    medium = g.make_constant_medium(g.make_sphere((0, 0, 0), 1, red), 0.5, g.constant_texture((1, 1, 1)))
    for other in (curve, g.make_klein((0, 0, 0), red), medium):
        with pytest.raises(RtError, match="cannot hold a curve, a Klein set or a constant medium"):
            gpu.upload(g.make_scene([tri, other], cam, g.sky_color))
    with pytest.raises(RtError, match="boundary"):
        gpu.upload(g.make_scene([g.make_constant_medium(tri, 0.5, g.constant_texture((1, 1, 1)))], cam, g.sky_color))
    sc = g.make_scene([tri], cam, g.sky_color)
    # (make_scene refuses it on the Python side, and through the ABI rt_set_light_sampling's older check fires
    # before the commit: build_scene's own message, for a scene description filled directly, is asserted in
    # tests/csrc/tri_check.cpp)
    sc.light = tri
    with pytest.raises(RtError, match="rect or a sphere|light-sampling target"):
        gpu.upload(sc)
    # a committed scene takes no more triangles
    import ctypes
    from rtamd import _lib
    h = gpu.upload(g.make_scene([tri], cam, g.sky_color))
    dv, out = _lib.dvec, ctypes.c_int(0)
    assert _lib.lib().rt_add_triangle(h, dv((0, 0, 0)), dv((1, 0, 0)), dv((0, 1, 0)), 0, ctypes.byref(out)) != 0
    assert b"already committed" in _lib.lib().rt_last_error()
