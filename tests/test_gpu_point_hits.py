"""Point records for the lambertian hit queue (rt_device.h HitPt): the SOLO LDS kernels queue a
lambertian hit as the hit point instead of t, and the lambertian shade's PT instances read no ray.  The point
is formed with hit_record's own expression on the same operands, so every image must equal, bit for bit, the
one rendered with RTAMD_NO_POINT_HITS=1 (t records everywhere); rt_scene_point_hits says which path a scene's
renders take, so each comparison asserts that both paths really ran.

Every render: 160x96, 8 spp, two lanes, max_paths = 4 * nx * ny — two chunks of 61 440 paths, above the
32 768-path tail floor, so depth 0 runs k_camera and the first depths k_extend_lds, over several blocks, all
eight shards and both lanes.
"""
import numpy as np
import pytest

from conftest import host_threads
from rtamd import gpu, scenes
from rtamd import scene as g
from rtamd import vec as v
from test_gpu_parity import RMS_TOL, _compare

pytestmark = pytest.mark.gpu

NX, NY, SPP = 160, 96, 8
SEED = 0x5EED0002
SWITCHES = ("RTAMD_NO_POINT_HITS", "RTAMD_NO_CAMERA_LDS", "RTAMD_NO_EXTEND_LDS", "RTAMD_NO_SOLO", "RTAMD_BVH_MIN")

_images = {}            # (scene, tail_off, libm, switches) -> (image, probe): each render is made once


def _render(ctx, monkeypatch, name, tail_off=False, libm="auto", env=()):
    key = (name, tail_off, libm, tuple(sorted(env)))
    if key in _images:
        return _images[key]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k in env:                               # "NAME" (set to 1) or "NAME=value"
        monkeypatch.setenv(*(k.split("=") if "=" in k else (k, "1")))
    ctx.reset_options()
    ctx.set_option("lanes", 2)
    ctx.set_option("max_paths", 4 * NX * NY)
    ctx.set_option("tail_off", 1 if tail_off else 0)
    ctx.set_option("exact_libm", libm)
    scene = SCENE_MAKERS[name](NX, NY)          # a new scene object: the LDS and SOLO switches are read at its commit
    acc = np.zeros(NX * NY * 3)
    h = gpu.render_host(scene, NX, NY, 0, SPP, SEED, acc, ctx=ctx)
    st = gpu.stats(h)
    assert (st.chunks, st.lanes) == (2, 2)
    assert st.shade_hits_d0 > 0 and (st.shade_hits > 0 or st.finish_paths > 0)
    if tail_off:
        assert st.finish_paths == 0
    assert np.isfinite(acc).all()
    _images[key] = (acc, gpu.point_hits(h), scene)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return _images[key]


def front_moving_sphere(nx, ny):
    """A ground sphere and one large lambertian sphere that moves during the shutter, in front of the camera:
    most camera rays end in a moving-sphere lambertian hit at a time other than 0."""
    ground = g.make_sphere(v.vec3(0, -1000, 0), 1000, g.make_lambertian(g.constant_texture(v.vec3(0.5, 0.5, 0.5))))
    ball = g.make_moving_sphere(v.vec3(0, 1, 0), v.vec3(0.4, 1.6, 0.2), 0, 1, 1.0,
                                g.make_lambertian(g.constant_texture(v.vec3(0.7, 0.3, 0.2))))
    return g.make_scene([ball, ground], scenes.camera_for(nx, ny), g.sky_color)


SCENE_MAKERS = {"cover": scenes.random_scene, "cover_marble": scenes.marble_random_scene,
                "cornell": scenes.cornell_box, "front_moving_sphere": front_moving_sphere}


@pytest.mark.parametrize("tail_off", [True, False], ids=["wavefront", "tail"])
@pytest.mark.parametrize("libm", ["exact", "device"])
@pytest.mark.parametrize("name", ["cover", "cover_marble"])
def test_bitwise_against_switch(sched, monkeypatch, name, libm, tail_off):
    """Point records against t records, every depth in the wavefront and with the production tail, both libm
    modes.  The cover scenes' small spheres move and the camera's shutter is [0, 1], so depth-0 lambertian
    hits on moving spheres at times other than 0 are in them."""
    a, on, _ = _render(sched, monkeypatch, name, tail_off, libm)
    b, off, _ = _render(sched, monkeypatch, name, tail_off, libm, env=("RTAMD_NO_POINT_HITS",))
    assert on is True and off is False
    assert np.array_equal(a, b)


@pytest.mark.parametrize("tail_off", [True, False], ids=["wavefront", "tail"])
@pytest.mark.parametrize("switch", ["RTAMD_NO_CAMERA_LDS", "RTAMD_NO_EXTEND_LDS"])
def test_mixed_formats_in_one_render(sched, monkeypatch, switch, tail_off):
    """With one LDS kernel off, that depth range's launches (k_raygen + k_extend at depth 0, or k_extend
    deeper) write t records and the other's point records, in one render."""
    a, on, _ = _render(sched, monkeypatch, "cover", tail_off)
    b, mixed, _ = _render(sched, monkeypatch, "cover", tail_off, env=(switch,))
    assert on is True and mixed is True
    assert np.array_equal(a, b)


@pytest.mark.parametrize("name,env", [("cover", ("RTAMD_NO_SOLO",)), ("cornell", ())], ids=["no_solo", "cornell"])
def test_scenes_that_must_not_take_it(sched, monkeypatch, name, env):
    """A world that is not one sphere BVH of direct leaves (RTAMD_NO_SOLO; the Cornell box's rects and
    instanced boxes) keeps t records, and the switch changes nothing in it."""
    a, pa, _ = _render(sched, monkeypatch, name, True, env=env)
    b, pb, _ = _render(sched, monkeypatch, name, True, env=env + ("RTAMD_NO_POINT_HITS",))
    assert pa is False and pb is False
    assert np.array_equal(a, b)


def test_front_moving_sphere_parity(sched, monkeypatch, oracle_mod):
    """The purpose-built scene against the oracle, within the small parity tests' bound (test_gpu_parity)."""
    acc, on, scene = _render(sched, monkeypatch, "front_moving_sphere", True, env=("RTAMD_BVH_MIN=1",))
    assert on is True
    ref, _ = oracle_mod.build_scene(scene).render(NX, NY, 0, SPP, SEED, nthreads=host_threads())
    rms, dmax, nbad, npx = _compare(acc, ref, SPP)
    print("front_moving_sphere: rms=%.3e max=%.3e pixels>1e-9: %d/%d" % (rms, dmax, nbad, npx))
    assert rms <= RMS_TOL
    assert nbad <= max(2, npx // 200)
