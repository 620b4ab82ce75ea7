"""GPU parity tests: librtamd's HIP path vs the oracle (C f64 restatement of
the reference), same scenes, same counter RNG streams.

The gate (BASELINE.json north_star): per-pixel linear-RGB RMS of sum/spp
<= 1e-4.  Both sides compute in f64 with the same operation order, so
differences come only from libm-vs-OCML transcendental ulps (sin, cos, pow)
and FMA contraction; in practice almost every pixel agrees to ~1e-12.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import host_threads
from hit_ray_cases import many_spheres_scene as _many_spheres_scene
from hit_ray_cases import moving_mix_scene as _moving_mix_scene
from hit_ray_cases import static_cover_scene as _static_cover_scene
from rtamd import gpu, scenes
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4          # north_star per-pixel RGB RMS tolerance
SEED = 0x5EED0002


def _compare(acc_gpu, acc_orc, spp):
    a = acc_gpu / spp
    b = acc_orc / spp
    d = np.abs(a - b)
    rms = float(np.sqrt(np.mean((a - b) ** 2)))
    px = d.reshape(-1, 3).max(axis=1)
    return rms, float(d.max()), int((px > 1e-9).sum()), px.size


def _both(scene, nx, ny, spp, oracle_mod, spp_begin=0, seed=SEED):
    acc = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, spp_begin, spp, seed, acc)
    o = oracle_mod.build_scene(scene)
    ref, _ = o.render(nx, ny, spp_begin, spp, seed, nthreads=host_threads())
    return acc, ref


@pytest.mark.parametrize("name,nx,ny,spp", [
    ("cover", 96, 54, 8),
    ("cover_marble", 64, 36, 4),
    ("test_scene", 64, 48, 8),
    ("test_scene2", 64, 48, 8),
    ("cornell", 48, 48, 16),
    ("bvh_sah", 64, 36, 4),
    ("test_bezier", 64, 36, 4),
    ("cornell_bezier", 48, 48, 8),
    ("curves_small", 64, 36, 2),
    ("cornell_smoke", 48, 48, 8),
    ("cornell_klein", 32, 32, 2),
    ("cornell_mixture", 48, 48, 8),
])
def test_scene_parity(name, nx, ny, spp, gpu_ctx, oracle_mod):
    scene = scenes.SCENES[name](nx, ny)
    acc, ref = _both(scene, nx, ny, spp, oracle_mod)
    rms, dmax, nbad, npx = _compare(acc, ref, spp)
    print("%s: rms=%.3e max=%.3e pixels>1e-9: %d/%d" % (name, rms, dmax, nbad, npx))
    assert np.isfinite(acc).all()
    assert rms <= RMS_TOL
    # ulp-level agreement for the overwhelming majority of pixels
    assert nbad <= max(2, npx // 200)


def test_full_width_band_parity(sched, oracle_mod):
    """Config C2 geometry (1920x1080, aspect 16/9) on a band of rows."""
    nx, ny, spp = 1920, 1080, 2
    scene = scenes.random_scene(nx, ny)
    acc = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, spp, SEED, acc)
    o = oracle_mod.build_scene(scene)
    lo, hi = 500 * nx, 508 * nx          # rows 500..507 (horizon region)
    ref = np.zeros(nx * ny * 3)
    o.render(nx, ny, 0, spp, SEED, ref, lo, hi, nthreads=host_threads())
    rms, dmax, nbad, npx = _compare(acc[3 * lo:3 * hi], ref[3 * lo:3 * hi], spp)
    print("band: rms=%.3e max=%.3e bad=%d/%d" % (rms, dmax, nbad, npx))
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 200)
    # every pixel of the frame was written and is finite
    assert np.isfinite(acc).all() and (acc.reshape(-1, 3).sum(axis=1) > 0).mean() > 0.99


def _schedule(ctx, schedule):
    """"wavefront": the tail kernel off, so every depth runs through k_camera /
    k_extend_lds / k_shade with sharded compaction (these small renders would
    otherwise fit under the tail threshold and run in k_finish only)."""
    if schedule == "wavefront":
        ctx.set_option("tail_off", 1)


SCHEDULES = ["tail", "wavefront"]


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_accumulate_across_calls_bitwise(sched, monkeypatch, schedule):
    """spp passes in one call == the same passes split over calls (trace-all
    running sum, main.scm:480)."""
    _schedule(sched, schedule)
    nx, ny = 40, 30
    scene = scenes.random_scene(nx, ny)
    a = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, 6, SEED, a)
    b = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, 2, SEED, b)
    gpu.render_host(scene, nx, ny, 2, 4, SEED, b)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_batching_independent_bitwise(sched, monkeypatch, schedule):
    """Results do not depend on the path-pool size (chunking of samples)."""
    _schedule(sched, schedule)
    nx, ny = 50, 20
    scene = scenes.cornell_box(nx, ny)
    a = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, 8, SEED, a)
    sched.set_option("max_paths", 1024)
    b = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, 8, SEED, b)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_lanes_and_chunks_bitwise(sched, monkeypatch, lanes, schedule):
    """Overlapped path pools (lanes) and many small chunks give the one-chunk
    image bit for bit: chunks are accumulated in sample order whichever lane
    finishes first."""
    _schedule(sched, schedule)
    nx, ny, spp = 48, 40, 12
    scene = scenes.random_scene(nx, ny)
    a = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, spp, SEED, a)
    sched.set_option("max_paths", nx * ny * 2)   # 6 chunks of 2 spp
    sched.set_option("lanes", int(lanes))
    b = np.zeros(nx * ny * 3)
    gpu.render_host(scene, nx, ny, 0, spp, SEED, b)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_shards_union_bitwise(sched, monkeypatch, schedule):
    """Interleaved tile shards (the multi-GPU partition) reassemble the
    single-device image bit for bit."""
    _schedule(sched, schedule)
    import torch
    nx, ny, spp = 70, 45, 3
    scene = scenes.random_scene(nx, ny)
    full = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    gpu.render_device(scene, nx, ny, 0, spp, SEED, full.data_ptr())
    parts = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    for r in range(4):
        gpu.render_device(scene, nx, ny, 0, spp, SEED, parts.data_ptr(), shard=r, nshard=4)
    torch.cuda.synchronize()
    assert torch.equal(full, parts)


def test_trace_all_passes_match_oracle_image(sched, oracle_mod):
    """Renderer.trace_all pass by pass (main.scm:471-491) and the u8 image."""
    from rtamd.render import Renderer
    nx, ny = 32, 24
    scene = scenes.test_scene(nx, ny)
    r = Renderer(nx, ny, seed=SEED)
    for k in (1, 2, 3):
        img = r.trace_all(scene, k)
    o = oracle_mod.build_scene(scene)
    ref, _ = o.render(nx, ny, 0, 3, SEED)
    ref_img = oracle_mod.resolve_u8(ref, 3)
    diff = np.abs(img.astype(int) - ref_img.astype(int))
    assert diff.max() <= 1 and (diff > 0).sum() <= 2


def test_edge_sizes(sched, oracle_mod):
    for nx, ny in ((1, 1), (17, 3), (3, 17)):
        scene = scenes.test_scene(nx, ny)
        acc, ref = _both(scene, nx, ny, 2, oracle_mod)
        rms, _, _, _ = _compare(acc, ref, 2)
        assert rms <= RMS_TOL


def test_zero_spp_is_noop(sched):
    nx, ny = 8, 8
    scene = scenes.test_scene(nx, ny)
    a = np.full(nx * ny * 3, 0.25)
    gpu.render_host(scene, nx, ny, 0, 0, SEED, a)
    assert (a == 0.25).all()


def test_errors_are_loud(sched):
    from rtamd._lib import RtError, call
    with pytest.raises(RtError):
        call("rt_render", 987654, 4, 4, 0, 1, ctypes.c_uint64(1), None)
    scene = scenes.test_scene(4, 4)
    with pytest.raises(ValueError):
        gpu.render_host(scene, 4, 4, 0, 1, SEED, np.zeros(4 * 4 * 3)[:-3])
    h = gpu.upload(scene)
    with pytest.raises(RtError):      # invalid shard
        call("rt_render_device", h, 4, 4, 0, 1, ctypes.c_uint64(1), 3, 2, ctypes.c_void_p(1), None)
    with pytest.raises(RtError):      # negative size
        call("rt_render", h, -4, 4, 0, 1, ctypes.c_uint64(1), np.zeros(48).ctypes.data_as(
            ctypes.POINTER(ctypes.c_double)))


def test_device_resolve_matches_host(sched):
    import torch
    nx, ny = 33, 21
    scene = scenes.random_scene(nx, ny)
    acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    gpu.render_device(scene, nx, ny, 0, 4, SEED, acc.data_ptr())
    out = torch.zeros(nx * ny * 3, dtype=torch.uint8, device="cuda")
    gpu.resolve_u8_device(acc.data_ptr(), nx, ny, 4, out.data_ptr(), ctx=sched)
    host = gpu.resolve_u8(acc.cpu().numpy(), nx, ny, 4)
    assert np.array_equal(out.cpu().numpy(), host)


def test_bvh_matches_flat_list_bitwise(sched, monkeypatch):
    """The BVH only culls: the image equals the brute-force flat list
    (geometry.scm:33-50) bit for bit."""
    nx, ny, spp = 64, 40, 4
    monkeypatch.setenv("RTAMD_BVH_MIN", "1000000000")
    flat_scene = scenes.random_scene(nx, ny)
    a = np.zeros(nx * ny * 3)
    gpu.render_host(flat_scene, nx, ny, 0, spp, SEED, a)
    monkeypatch.setenv("RTAMD_BVH_MIN", "1")
    bvh_scene = scenes.random_scene(nx, ny)
    b = np.zeros(nx * ny * 3)
    gpu.render_host(bvh_scene, nx, ny, 0, spp, SEED, b)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("wavefront", [False, True])
def test_sah_builders_same_image_bitwise(sched, monkeypatch, wavefront):
    """The exact-sweep SAH tree (default for sphere trees) and the binned
    one (RTAMD_BVH_SWEEP=0) only cull differently: same image, bit for bit,
    through the tail kernel and through the wavefront kernels."""
    nx, ny, spp = 64, 40, 4
    if wavefront:
        sched.set_option("tail_off", 1)
    imgs = []
    for sweep in ("0", None):
        if sweep is None:
            monkeypatch.delenv("RTAMD_BVH_SWEEP", raising=False)
        else:
            monkeypatch.setenv("RTAMD_BVH_SWEEP", sweep)
        a = np.zeros(nx * ny * 3)
        gpu.render_host(scenes.random_scene(nx, ny), nx, ny, 0, spp, SEED, a)
        imgs.append(a)
    assert np.array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("make", [_static_cover_scene, _many_spheres_scene],
                         ids=["_static_cover_scene", "_many_spheres_scene"])
def test_kernel_paths_match_flat_list_bitwise(sched, monkeypatch, make):
    """Scenes that take the other closest-hit paths (time-0 tree for camera
    rays; trees too big for LDS) equal the brute-force flat list bit for bit."""
    nx, ny, spp = 48, 27, 4
    imgs = []
    for env in ({"RTAMD_BVH_MIN": "1000000000"}, {}):
        monkeypatch.delenv("RTAMD_BVH_MIN", raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        a = np.zeros(nx * ny * 3)
        gpu.render_host(make(nx, ny), nx, ny, 0, spp, SEED, a)
        imgs.append(a)
    assert np.array_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("make", [scenes.random_scene, _moving_mix_scene],
                         ids=["random_scene", "_moving_mix_scene"])
def test_time0_bvh_matches_all_times_bvh_bitwise(sched, monkeypatch, make):
    """Scattered rays (time 0) traverse the time-0 tree with moving spheres
    frozen at center(0); the image equals the one from the all-times tree and
    the flat list bit for bit."""
    nx, ny, spp = 64, 40, 4
    imgs = []
    for env in ({"RTAMD_BVH_MIN": "1000000000"}, {"RTAMD_NO_BVH0": "1"}, {}):
        for k in ("RTAMD_BVH_MIN", "RTAMD_NO_BVH0"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        a = np.zeros(nx * ny * 3)
        gpu.render_host(make(nx, ny), nx, ny, 0, spp, SEED, a)
        imgs.append(a)
    assert np.array_equal(imgs[0], imgs[1])
    assert np.array_equal(imgs[1], imgs[2])


@pytest.mark.parametrize("name", ["test_scene", "test_scene2", "cornell", "cover", "bvh_sah", "test_bezier",
                                  "cornell_bezier", "cornell_smoke", "klein", "cornell_klein"])
def test_gpu_vs_reference_fixtures(name, gpu_ctx):
    """The GPU against the outputs of the REFERENCE's own source, executed
    (tests/golden/make_golden.py): same scene, seed and streams."""
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_%s.json" % name)
    with open(path) as f:
        g = json.load(f)
    nx, ny, spp = g["nx"], g["ny"], g["spp"]
    want = np.array([float.fromhex(v) for px in g["accum"] for v in px])
    acc = np.zeros(nx * ny * 3)
    gpu.render_host(scenes.SCENES[name](nx, ny), nx, ny, 0, spp, g["path_seed"], acc)
    rms, dmax, nbad, npx = _compare(acc, want, spp)
    print("%s vs reference: rms=%.3e max=%.3e pixels>1e-9: %d/%d" % (name, rms, dmax, nbad, npx))
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 100)
    img = gpu.resolve_u8(acc, nx, ny, spp)
    assert (np.abs(img.astype(int) - np.array(g["image"])) <= 1).all()


def test_curve_bvh_matches_flat_list_bitwise(sched, monkeypatch):
    """Curves in the BVH (boxes = control points +- width/2, t range widened
    for |dir| < 1 rays, Q10) give the flat list's image bit for bit."""
    nx, ny, spp = 64, 36, 2
    monkeypatch.setenv("RTAMD_BVH_MIN", "1000000000")
    a = np.zeros(nx * ny * 3)
    gpu.render_host(scenes.cornell_curves_small(nx, ny), nx, ny, 0, spp, SEED, a)
    monkeypatch.setenv("RTAMD_BVH_MIN", "1")
    b = np.zeros(nx * ny * 3)
    gpu.render_host(scenes.cornell_curves_small(nx, ny), nx, ny, 0, spp, SEED, b)
    assert np.array_equal(a, b)


def test_media_in_list_order(sched, oracle_mod):
    """A medium listed between other objects (and a sphere-bounded one, and
    one under an instance) draws its random number with the closest hit of
    the objects before it only: GPU vs oracle."""
    from rtamd import scene as g
    from rtamd.camera import make_camera
    white = g.make_lambertian(g.constant_texture((0.73, 0.73, 0.73)))
    red = g.make_lambertian(g.constant_texture((0.65, 0.05, 0.05)))
    light = g.make_diffuse_light(g.constant_texture((4, 4, 4)))
    objs = [
        g.make_sphere((0, -1000, 0), 1000, white),
        g.make_constant_medium(g.make_sphere((0, 1, 0), 1, white), 0.8, g.constant_texture((0.2, 0.4, 0.9))),
        g.make_sphere((1.2, 0.7, 0.5), 0.7, red),
        g.translate(g.rotate_y(g.make_constant_medium(g.make_box((0, 0, 0), (1, 1, 1), white), 1.5,
                                                      g.constant_texture((0.9, 0.9, 0.9))), 30), (-2, 0, 0)),
        g.make_xz_rect(-3, 3, -3, 3, 5, light),
    ]
    sc = g.make_scene(objs, make_camera((0, 2, 6), (0, 0.5, 0), (0, 1, 0), 50, 1.5, 0, 1, 0, 1), g.sky_color)
    nx, ny, spp = 60, 40, 8
    acc, ref = _both(sc, nx, ny, spp, oracle_mod)
    rms, dmax, nbad, npx = _compare(acc, ref, spp)
    print("media order: rms=%.3e max=%.3e pixels>1e-9: %d/%d" % (rms, dmax, nbad, npx))
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 200)


def test_sphere_light_mixture(sched, oracle_mod):
    """pdf.scm mixture toward a sphere light (extension f2): GPU vs oracle."""
    from rtamd import scene as g
    from rtamd.camera import make_camera
    lam = g.make_lambertian(g.constant_texture((0.6, 0.5, 0.4)))
    light = g.make_sphere((0, 3, 0), 0.7, g.make_diffuse_light(g.constant_texture((4, 4, 4))))
    sc = g.make_scene([g.make_sphere((0, -1000, 0), 1000, lam), g.make_sphere((0, 1, 0), 1, lam), light],
                      make_camera((0, 1.5, 6), (0, 1, 0), (0, 1, 0), 40, 1.5, 0, 1, 0, 1), g.black, light=light)
    nx, ny, spp = 60, 40, 8
    acc, ref = _both(sc, nx, ny, spp, oracle_mod)
    rms, dmax, nbad, npx = _compare(acc, ref, spp)
    print("sphere-light mixture: rms=%.3e max=%.3e pixels>1e-9: %d/%d" % (rms, dmax, nbad, npx))
    assert np.isfinite(acc).all()
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 200)


def test_c_example_matches_python_host(sched, tmp_path):
    """The C-ABI example (examples/cornell.c) and the Python host render the
    same cornell-box to the same PPM bytes."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_host import _build_c_example
    from rtamd import render
    nx, ny, spp = 64, 48, 4
    exe = _build_c_example(tmp_path)
    ppm_c = tmp_path / "c.ppm"
    subprocess.run([str(exe), str(nx), str(ny), str(spp), str(ppm_c)], check=True, timeout=300)
    acc = np.zeros(nx * ny * 3)
    gpu.render_host(scenes.cornell_box(nx, ny), nx, ny, 0, spp, SEED, acc)
    ppm_py = tmp_path / "py.ppm"
    render.write_ppm(str(ppm_py), gpu.resolve_u8(acc, nx, ny, spp), nx, ny)
    assert ppm_c.read_bytes() == ppm_py.read_bytes()
    # the multi-GPU frame's path from C at world size 1: rt_render_shard_device + rt_gather_shards
    ppm_g = tmp_path / "g.ppm"
    subprocess.run([str(exe), str(nx), str(ny), str(spp), str(ppm_g), "gather"], check=True, timeout=300)
    assert ppm_g.read_bytes() == ppm_py.read_bytes()


_WAVEFRONT_SCENES = ["cover", "cover_marble", "test_scene2", "cornell", "cornell_mixture", "cornell_smoke",
                     "bvh_sah", "cornell_bezier", "curves_small", "cornell_klein"]


@pytest.mark.parametrize("name", _WAVEFRONT_SCENES)
def test_wavefront_matches_tail_kernel_bitwise(sched, monkeypatch, name):
    """Small renders run entirely in the tail kernel (k_finish: extend + shade
    per lane).  With the tail switched off the same render goes through the
    wavefront kernels (k_camera / raygen, k_extend_lds / k_extend<F> /
    k_extend_curves, the per-material k_shade queues) for every depth: the
    two images must agree bit for bit, for every closest-hit and material
    path the scenes reach."""
    nx, ny, spp = 40, 24, 3
    if name.startswith("curves") or "bezier" in name:
        nx, ny, spp = 32, 18, 2
    sched.set_option("tail_off", 0)
    a = np.zeros(nx * ny * 3)
    gpu.render_host(scenes.SCENES[name](nx, ny), nx, ny, 0, spp, SEED, a)
    sched.set_option("tail_off", 1)
    b = np.zeros(nx * ny * 3)
    gpu.render_host(scenes.SCENES[name](nx, ny), nx, ny, 0, spp, SEED, b)
    assert np.isfinite(a).all()
    assert np.array_equal(a, b), np.abs(a - b).max()


@pytest.mark.parametrize("libm", ["exact", "device"])
def test_fused_curve_extend_bitwise(sched, monkeypatch, libm):
    """The fused curve extend (k_extend_curves<FUSE>: every depth >= 1 in one launch, hits shaded in the
    kernel) in both libm instances (FUSE 2: the exact sin / cos; FUSE 1: the device's) against one launch
    per depth with the wavefront shade kernels, on a scene with every material (lambertian curves and
    walls, metal, glass, a light, moving spheres) at a production-sized launch (2 lanes, 4 chunks): the
    same image bit for bit, and the same segment count."""
    from rtamd import scene as g, vec as v
    from rtamd.rng import HostStream
    nx, ny, spp = 320, 240, 8
    rr = HostStream(0x5EED0105)
    red = g.make_lambertian(g.constant_texture(v.vec3(0.65, 0.05, 0.05)))
    white = g.make_lambertian(g.constant_texture(v.vec3(0.73, 0.73, 0.73)))
    metal = g.make_metal(g.constant_texture(v.vec3(0.8, 0.8, 0.7)), 0.1)
    glass = g.make_dielectric(1.5)
    light = g.make_diffuse_light(g.constant_texture(v.vec3(4, 4, 4)))
    objs = [g.flip_normals(g.make_yz_rect(0, 555, 0, 555, 555, white)), g.make_xz_rect(0, 555, 0, 555, 0, white),
            g.bezier_array(scenes.random_polyline_curves(2000), 3.0, red)]
    for i in range(30):
        c = v.vec3(60 + rr() * 430, 40 + rr() * 400, 60 + rr() * 430)
        m = (white, metal, glass)[i % 3]
        if i % 4 == 0:
            objs.append(g.make_moving_sphere(c, v.vec3(c[0], c[1] + 20, c[2]), 0.0, 1.0, 15 + 10 * rr(), m))
        else:
            objs.append(g.make_sphere(c, 10 + 15 * rr(), m))
    objs += [g.flip_normals(g.make_xz_rect(213, 343, 227, 332, 554, light)), g.make_yz_rect(0, 555, 0, 555, 0, red)]
    sc = g.make_scene(objs, scenes.cornell_camera_for(nx, ny), g.sky_color)
    sched.set_option("exact_libm", libm)
    sched.set_option("lanes", 2)
    sched.set_option("max_paths", nx * ny * 2)           # 4 chunks of 2 spp, each far above the tail threshold
    imgs, segs = [], []
    for fuse in ("1", "0"):
        monkeypatch.setenv("RTAMD_CURVE_FUSE", fuse)
        a = np.zeros(nx * ny * 3)
        h = gpu.render_host(sc, nx, ny, 0, spp, SEED, a)
        st = gpu.stats(h)
        imgs.append(a)
        segs.append(st.segments)
        if fuse == "1":
            assert st.shade_hits == 0 and st.finish_paths == 0     # depths >= 1 ran fused, no tail kernel
        else:
            assert st.shade_hits > 0
    print("fused curve extend (%s libm): segments %d / %d" % (libm, segs[0], segs[1]))
    assert np.isfinite(imgs[0]).all() and imgs[0].any()
    assert np.array_equal(imgs[0], imgs[1]), np.abs(imgs[0] - imgs[1]).max()
    assert segs[0] == segs[1]


@pytest.mark.parametrize("flat_curves", [False, True])
def test_curve_kernels_bitwise(sched, monkeypatch, flat_curves):
    """Curves, spheres and moving spheres in one world BVH between rect
    groups, through the wavefront: the persistent curve extend (fused over the
    depths, and one launch per depth), the per-ray curve kernel and the flat
    list give the same image bit for bit.
    flat_curves adds short, nearly straight curves whose subdivision depth
    ceil(log4(...)) is negative (bezier.scm:180-193: the root is a leaf); the
    flat list's per-lane test and the batched stage A/B must agree on them.
    (The C5 fault that the leaf-level clamp fixed did not reproduce at this
    size, so this is a parity check for the case, not that fault's replay.)"""
    import curve_step_cases
    nx, ny, spp = 40, 40, 2
    sc = curve_step_cases.curve_mix_scene(nx, ny, flat_curves)      # (the step probe's records run on it too)
    sched.set_option("tail_off", 1)
    imgs = []
    # the flat list, the per-ray kernel, the persistent curve extend fused over the depths (the default: hits
    # shaded in the kernel, every material of the scene; also with 3 blocks), and one launch per depth
    # (RTAMD_CURVE_FUSE=0, also with 3 blocks)
    for env in ({"RTAMD_BVH_MIN": "1000000000"}, {"RTAMD_CURVE_BLOCKS": "0"}, {}, {"RTAMD_CURVE_BLOCKS": "3"},
                {"RTAMD_CURVE_FUSE": "0"}, {"RTAMD_CURVE_FUSE": "0", "RTAMD_CURVE_BLOCKS": "3"}):
        for k in ("RTAMD_BVH_MIN", "RTAMD_CURVE_BLOCKS", "RTAMD_CURVE_FUSE"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        a = np.zeros(nx * ny * 3)
        gpu.render_host(sc, nx, ny, 0, spp, SEED, a)
        imgs.append(a)
    assert np.isfinite(imgs[0]).all()
    for a in imgs[1:]:
        assert np.array_equal(imgs[0], a), np.abs(imgs[0] - a).max()


@pytest.mark.parametrize("name", ["cover", "cornell", "test_bezier", "cornell_bezier", "curves_small", "cornell_klein",
                                  "bvh_sah"])
def test_hit_rays_vs_oracle_hit_world(sched, oracle_mod, name):
    """rt_hit_rays (the extend kernels' closest_hit on a caller's rays) against
    the oracle's hit-obj-list over the same scene list (orc_hit_world): camera
    and scattered-like rays, unit and raw directions, |dir| < 1, times 0 and
    inside the shutter.  Same t bit for bit and the same material."""
    nx, ny = 64, 36
    sc = scenes.SCENES[name](nx, ny)
    o = oracle_mod.build_scene(sc)
    rng = np.random.default_rng(0x5EED0201)
    cam = np.array(sc.camera.slots())
    n = 4096
    # camera rays through random film points, then rays from random points inside the scene's box
    s_, t_ = rng.uniform(0, 1, n // 2), rng.uniform(0, 1, n // 2)
    d0 = cam[0:3] + s_[:, None] * cam[3:6] + t_[:, None] * cam[6:9] - cam[9:12]
    o0 = np.broadcast_to(cam[9:12], d0.shape)
    tm0 = cam[22] + rng.uniform(0, 1, n // 2) * (cam[23] - cam[22])
    lo, hi = (np.array([0.0, 0.0, 0.0]), np.array([555.0, 555.0, 555.0])) if "cornell" in name else \
        (np.array([-6.0, 0.0, -4.0]), np.array([10.0, 3.0, 10.0]))
    o1 = rng.uniform(lo, hi, (n // 2, 3))
    d1 = rng.normal(size=(n // 2, 3))
    d1[::3] /= np.linalg.norm(d1[::3], axis=1)[:, None]
    d1[1::3] *= 0.3
    rays = np.zeros((n, 7))
    rays[:n // 2, 0:3], rays[:n // 2, 3:6], rays[:n // 2, 6] = o0, d0, tm0
    rays[n // 2:, 0:3], rays[n // 2:, 3:6] = o1, d1
    t, m = gpu.hit_rays(sc, rays)
    bad = []
    hits = 0
    for k in range(n):
        h = o.hit_world(rays[k, 0:3], rays[k, 3:6], rays[k, 6])
        et, em = (h[0], int(h[7])) if h else (0.0, -1)
        hits += h is not None
        if et != t[k] or em != m[k]:
            bad.append((k, et, em, t[k], m[k]))
    print("%s: %d rays, %d hits, %d differ" % (name, n, hits, len(bad)), bad[:3])
    assert hits > n // 8
    assert len(bad) <= n // 1000, bad[:5]


def test_hit_rays_refuses_media(sched):
    with pytest.raises(RtError, match="media"):
        gpu.hit_rays(scenes.cornell_smoke(16, 16), np.zeros((1, 7)))
