"""Per-vertex shading normals on the GPU (RT_HAS_SMOOTH_NORMALS), on the scenes of tests/smooth_cases.py.

The truth for a hit record's normal is rtamd.mesh.shading_normal (the NumPy restatement of include/rt.h's
"shading normals") on the hit rtamd.mesh.hit finds, bit for bit; for a scatter from such a normal it is
smooth_cases.scatter, which test_smooth_normals_host.py pins to the oracle's orc_step on the shapes the oracle
holds.  All frames are 48x48."""
import functools

import numpy as np
import pytest
import torch

import mesh_cases as mc
import smooth_cases as sm
from rtamd import denoise, gpu, mesh, scenes
from rtamd import scene as g

pytestmark = pytest.mark.gpu

SEED = sm.SEED
NX, NY = sm.NX, sm.NY


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _features(scene, passes, first=0):
    feat = np.zeros(NX * NY * 8)
    gpu.render_features_host(scene, NX, NY, first, passes, SEED, feat)
    return feat.reshape(-1, 8)


def _render(scene, passes, seed=SEED):
    acc = np.zeros(NX * NY * 3)
    h = gpu.render_host(scene, NX, NY, 0, passes, seed, acc)
    return acc, gpu.stats(h)


# ------------------------------------------------------------------ 1. features, bit for bit
def test_features_of_a_flipped_instanced_smooth_ball(sched):
    """icosphere(1) with radial normals under flip + rotate-y 37 + translate, beside a plain quad, 4 passes: all
    eight channels equal the prediction (the oracle's camera rays, mesh.hit, shading_normal, the flip,
    out_of_instance) as uint64; and the prediction is not the flat one, so a library that ignores the normals fails."""
    passes = 4
    sc = sm.flipped_ball_scene()
    want, _, _, hit, which = sm.mesh_features(sc, passes)
    flat = sm.mesh_features(sc, passes, smooth=False)[0]
    differ = int((want[:, 3:6] != flat[:, 3:6]).any(axis=1).sum())
    got = _features(sc, passes)
    diff = got.view(np.uint64) != want.view(np.uint64)
    print("flipped smooth ball: %d of %d values differ; samples on the ball %d, on the quad %d, of %d; the flat "
          "prediction differs on %d pixels" % (diff.sum(), diff.size, (which == 0).sum(), (which == 1).sum(), hit.size, differ))
    assert differ > 100
    assert (which == 0).sum() > 400 and (which == 1).sum() > 400 and (which < 0).sum() > 400
    assert np.array_equal(want[:, [0, 1, 2, 6, 7]], flat[:, [0, 1, 2, 6, 7]])      # only the normal changes
    assert not diff.any(), np.argwhere(diff)[:8]


# ------------------------------------------------------------------ 2. the sphere bound on the device
def test_smooth_icosphere_has_the_sphere_normal(sched):
    """icosphere(3) with radial normals, 1 pass: with pt = o + d t from the camera ray, the feature normal is
    within 1e-12 of unit(pt - c) on every hit pixel (1000 x the 1.1e-15 measured with NumPy)."""
    c = np.array((0.25, 0.5, -0.5))
    vs, fs = mesh.icosphere(3, radius=1.5, center=tuple(c))
    ball = g.make_mesh(vs, fs, g.make_metal(g.constant_texture((0.8, 0.85, 0.88)), 0.0), normals=mesh.radial_normals(vs, c))
    got = _features(g.make_scene([ball], mc._cam(), g.sky_color), 1)
    rays, _ = sm.camera_rays(1)
    hit = got[:, 7] == 1.0
    pt = rays[hit, 0:3] + rays[hit, 3:6] * got[hit, 6:7]
    want = mesh.unit_normals(pt - c)
    dev = np.abs(got[hit, 3:6] - want).max(axis=1)
    flat = mesh.normal(vs[fs])
    geo = np.abs(flat[mesh.hit(vs[fs], rays[hit])[1]] - want).max(axis=1)
    print("smooth icosphere(3) on the device: %d hit pixels, normal off the radial direction by at most %.3e; the "
          "geometric normal by %.4f in the median" % (hit.sum(), dev.max(), np.median(geo)))
    assert hit.sum() >= 200 and (~hit).sum() > 100
    assert dev.max() <= 1e-12
    assert np.median(geo) > 0.01
    assert (got[~hit, 3:6] == 0.0).all()


# ------------------------------------------------------------------ 3. flat equivalence
@functools.lru_cache(maxsize=None)
def _cornell_mesh_with_face_normals():
    """cornell_mesh with each mesh's vertex normals set to mesh.normal of its faces (its vertices are per face)."""
    sc = scenes.SCENES["cornell_mesh"](NX, NY)

    def with_normals(o):
        if o.kind in ("flip", "translate", "rotate_y"):
            return g.Hitable(o.kind, with_normals(o.args[0]), *o.args[1:])
        vs, fs, uvs, mat = o.args
        fn = mesh.normal(vs[fs])
        ns = np.zeros_like(vs)
        for f in range(len(fs)):
            for k in range(3):
                assert not ns[fs[f, k]].any() or np.array_equal(ns[fs[f, k]], fn[f])   # one plane per vertex
                ns[fs[f, k]] = fn[f]
        return g.make_mesh(vs, fs, mat, uvs, normals=ns)
    return g.make_scene([with_normals(o) for o in sc.obj_list], sc.camera, sc.sky_function)


def test_face_normals_as_vertex_normals_render_the_flat_scene(sched):
    """The rule returns equal axis-aligned normals exactly (up to the sign of a zero, which only ever meets a
    nonzero addend in this scene's lambertian and light materials): the frames are equal, in every schedule."""
    flat, smooth = scenes.SCENES["cornell_mesh"](NX, NY), _cornell_mesh_with_face_normals()
    assert all(lf.obj.normals is not None for lf in mc.leaves_of(smooth)) and len(mc.leaves_of(smooth)) == 8
    base, st = _render(flat, 16)
    got, st2 = _render(smooth, 16)
    assert np.isfinite(base).all() and base.sum() > 0
    assert np.array_equal(got, base) and st2.segments == st.segments and st2.paths == st.paths
    sched.set_option("tail_off", 1)
    off, st3 = _render(smooth, 16)
    assert np.array_equal(off, base) and st3.segments == st.segments
    sched.reset_options()
    sched.set_option("lanes", 2)
    sched.set_option("max_paths", 4096)
    two, st4 = _render(smooth, 16)
    print("lanes/chunks:", st4.lanes, st4.chunks, "segments", st.segments)
    assert st4.lanes == 2 and st4.chunks > 2
    assert np.array_equal(two, base) and st4.segments == st.segments


# ------------------------------------------------------------------ 4. scatter, bit for bit
@pytest.mark.parametrize("name,material", [
    ("metal fuzz 0", g.make_metal(g.constant_texture((0.7, 0.6, 0.5)), 0.0)),
    ("metal fuzz 0.3", g.make_metal(g.constant_texture((0.8, 0.85, 0.88)), 0.3)),
    ("dielectric 1.5", g.make_dielectric(1.5)),
])
def test_scatter_from_the_shading_normal(sched, name, material):
    """rt_step_rays (one step, HBM extend, depth 1) on one smooth triangle with three distinct normals: the
    survivor's ray, throughput and counter, and the absorbed records, equal smooth_cases.scatter fed
    mesh.shading_normal at the restatement's hit point."""
    rays = sm.triangle_records()
    n = len(rays)
    T = sm.throughputs(n)
    ctr_in = (np.arange(n) * 5 % 23).astype(np.uint32)
    r = gpu.step_rays(sm.triangle_scene(material), rays, T_in=T, ctr_in=ctr_in, seed=SEED, smp=sm.SMP, depth=1,
                      extend=gpu.STEP_EXTEND_HBM, mode=gpu.STEP_STEP)
    t, idx = mesh.hit(sm.TRI[None], rays)
    hit = idx >= 0
    pt = rays[:, 0:3] + rays[:, 3:6] * t[:, None]
    nrm = mesh.shading_normal(sm.TRI, sm.TRI_NORMALS, pt)
    flat = mesh.normal(sm.TRI)
    entries, wrote = r.entries(), r.wrote()
    assert ((entries + wrote.astype(np.int32)) == 1).all()
    assert mc.hc.same_t(r.t, t).all() and np.array_equal(r.mat, np.where(hit, 0, -1))
    bad, survived, absorbed, flat_differs = [], 0, 0, 0
    for k in np.nonzero(hit)[0]:
        ok, o, d, a, c = sm.scatter(pt[k], nrm[k], rays[k], material, SEED, int(k), sm.SMP, int(ctr_in[k]))
        flat_differs += sm.scatter(pt[k], flat, rays[k], material, SEED, int(k), sm.SMP, int(ctr_in[k]))[2] != d
        if not ok:
            absorbed += 1
            if entries[k] != 0 or not wrote[k] or (r.color[k] != 0.0).any():
                bad.append((int(k), "absorbed"))
            continue
        survived += 1
        want_T = T[k] * np.array(a) if material.kind == "metal" else T[k]
        same = (entries[k] == 1 and np.array_equal(r.ray[k, 0:3].view(np.uint64), np.array(o).view(np.uint64))
                and np.array_equal(r.ray[k, 3:6].view(np.uint64), np.array(d).view(np.uint64))
                and np.array_equal(r.T[k].view(np.uint64), want_T.view(np.uint64)) and int(r.ctr[k]) == c)
        if not same:
            bad.append((int(k), "survivor", r.ray[k].tolist(), list(o) + list(d), int(r.ctr[k]), c))
    print("%s: %d records, %d hit, %d survive, %d absorbed, %d differ; the geometric normal would scatter %d otherwise; "
          "survivors counted %d" % (name, n, hit.sum(), survived, absorbed, len(bad), flat_differs, r.survivors))
    assert hit.sum() >= 500 and survived >= 300 and flat_differs >= 300                # (of 900: 300 per class)
    assert wrote[~hit].all()                                                     # a miss writes the sky
    assert r.survivors == survived
    assert not bad, bad[:4]


# ------------------------------------------------------------------ 5. unchanged behaviour
def test_a_mesh_without_normals_keeps_the_geometric_normal(sched):
    """The plain quad beside the smooth ball: its feature pixels hold mesh.normal of the face hit, exactly."""
    sc = sm.flipped_ball_scene()
    quad = mc.leaves_of(sc)[1]
    assert quad.obj.normals is None and mc.leaves_of(sc)[0].obj.normals is not None
    got = _features(sc, 1)
    rays, _ = sm.camera_rays(1)
    t, idx = mesh.hit(quad.tris, rays)
    on_quad = (idx >= 0) & (got[:, 7] == 1.0) & mc.hc.same_t(got[:, 6], t)       # (the ball is nowhere in front of it)
    want = mesh.normal(quad.tris)[idx[on_quad]]
    print("plain quad beside a smooth mesh: %d pixels" % on_quad.sum())
    assert on_quad.sum() > 100
    assert np.array_equal((got[on_quad, 3:6] + 0.0).view(np.uint64), (want + 0.0).view(np.uint64))


def test_a_smooth_image_textured_quad_shares_its_barycentrics(sched):
    """A quad with uvs, a 5x3 image and distinct vertex normals (the kTexImage instances, where hit_uv takes the
    barycentrics the shading normal formed) against the same quad without normals: albedo, t and hit flags equal
    bit for bit, the normals equal the prediction and differ from the flat ones."""
    rng = np.random.RandomState(5)
    data = rng.randint(0, 256, 5 * 3 * 3).astype(np.uint8)
    vs, fs, uvs = mesh.quad(*mc.QUAD)
    ns = np.array([[-0.4, 0.1, 1.0], [0.5, -0.2, 1.0], [0.3, 0.6, 1.0], [-0.2, 0.5, 0.7]])
    sc = {}
    for smooth in (True, False):
        m = g.make_lambertian(g.make_image_texture(data, 5, 3))
        sc[smooth] = g.make_scene([g.make_mesh(vs, fs, m, uvs, normals=ns if smooth else None)], mc._cam(), g.sky_color)
    a, b = _features(sc[True], 2), _features(sc[False], 2)
    want = sm.mesh_features(sc[True], 2)[0]
    hit = a[:, 7] > 0
    print("smooth image-textured quad: %d hit pixels, %d normals differ from the flat ones" %
          (hit.sum(), (a[hit, 3:6] != b[hit, 3:6]).any(axis=1).sum()))
    assert hit.sum() > 300 and len({tuple(x) for x in a[a[:, 7] == 2.0, 0:3]}) > 10
    assert np.array_equal(a[:, [0, 1, 2, 6, 7]].view(np.uint64), b[:, [0, 1, 2, 6, 7]].view(np.uint64))
    assert np.array_equal(a[:, 3:6].view(np.uint64), want[:, 3:6].view(np.uint64))
    assert (a[hit, 3:6] != b[hit, 3:6]).any(axis=1).sum() > 300


# ------------------------------------------------------------------ 6. adaptive render, denoiser
@functools.lru_cache(maxsize=None)
def _cornell_smooth():
    return scenes.SCENES["cornell_smooth"](NX, NY)


def test_adaptive_render_is_the_uniform_render_of_each_count(sched):
    sc = _cornell_smooth()
    lo, hi, step = 4, 12, 4
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
    print("adaptive on cornell_smooth:", res, np.bincount(cnt)[lo::step])
    assert set(np.unique(cnt)) <= set(range(lo, hi + 1, step)) and len(np.unique(cnt)) > 1
    assert np.array_equal(acc, S) and np.array_equal(acc2, Q)


def test_denoise_runs_on_a_smooth_mesh_scene(sched):
    passes, npx = 8, NX * NY
    sc = _cornell_smooth()
    S, Q = _dev(np.zeros(npx * 3)), _dev(np.zeros(npx * 3))
    cnt = _dev(np.zeros(npx, dtype=np.uint32))
    pix = _dev(gpu.shard_pixels(NX, NY, 0, 1))
    gpu.render_pixels_device(sc, NX, NY, pix.data_ptr(), npx, 0, passes, SEED, S.data_ptr(), Q.data_ptr(), cnt.data_ptr())
    feat = _dev(np.zeros(npx * 8))
    gpu.render_features_device(sc, NX, NY, 0, passes, SEED, feat.data_ptr())
    torch.cuda.synchronize()
    hS, hQ, hc, hf = S.cpu().numpy(), Q.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), feat.cpu().numpy()
    want = denoise.atrous(hS, hQ, hc, 0, hf, passes, NX, NY)
    d_o = _dev(np.full(npx * 3, -3.0))
    gpu.denoise_device(NX, NY, gpu.denoise_params(), S.data_ptr(), Q.data_ptr(), cnt.data_ptr(), 0, feat.data_ptr(),
                       passes, d_o.data_ptr())
    got = d_o.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print("denoise on cornell_smooth: max |device - numpy| = %.3e = %.3e * max |out|" % (err, err / scale))
    assert err <= 1e-12 * scale                                    # (test_gpu_denoise's bound)
    assert np.abs(want - hS / passes).max() > 1e-3                 # the filter did something
    # the ball's feature normals vary smoothly: no two of its pixels share a normal, as facets would make them
    f = hf.reshape(-1, 8)
    on_ball = (f[:, 7] == passes) & (np.abs(f[:, 0:3] / passes - np.array([0.8, 0.85, 0.88])).max(axis=1) < 1e-12)
    assert on_ball.sum() > 10 and len(np.unique(f[on_ball, 3:6], axis=0)) == on_ball.sum()
