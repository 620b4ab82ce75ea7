"""Image textures on the GPU (t:image-texture, texture.scm:36-50; include/rt.h, "image textures").

The oracle cannot hold an image texture, so each test rests on an equality the lookup rule implies:
an image whose texels are all one colour is that constant texture; an image on a rect is its split_rect twin
(one constant sub-rect per texel), which the oracle can render; a sphere's albedo feature is
rtamd.image.lookup at rtamd.image.sphere_uv of the oracle's first hit."""
import ctypes

import numpy as np
import pytest

import image_texture_cases as ic
import test_gpu_parity as parity
from conftest import host_threads
from rtamd import _lib, gpu, image, scenes

pytestmark = pytest.mark.gpu

SEED = ic.SEED


def _render(scene, nx, ny, spp, ctx=None):
    import torch
    acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    h = gpu.render_device(scene, nx, ny, 0, spp, SEED, acc.data_ptr(), ctx=ctx)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), gpu.stats(h)


def _features(scene, nx, ny, spp):
    feat = np.zeros(nx * ny * 8)
    gpu.render_features_host(scene, nx, ny, 0, spp, SEED, feat)
    return feat.reshape(nx * ny, 8)


def _apply(ctx, schedule, nx, ny):
    if schedule == "tail":
        ctx.set_option("tail_paths", 1 << 30)            # every depth >= 1 in the tail kernel
    elif schedule == "wavefront":
        ctx.set_option("tail_off", 1)                    # every depth through k_shade
    elif schedule == "chunks":
        ctx.set_option("max_paths", nx * ny * 2)         # 4 chunks of 2 passes on 2 lanes
        ctx.set_option("lanes", 2)
    elif schedule == "chunks_wavefront":
        ctx.set_option("max_paths", nx * ny * 2)
        ctx.set_option("lanes", 2)
        ctx.set_option("tail_off", 1)


# ------------------------------------------------------------------ 1. constant image == constant texture
@pytest.mark.parametrize("schedule", ["default", "tail", "wavefront", "chunks", "chunks_wavefront"])
def test_constant_images_equal_constant_textures_bitwise(sched, schedule):
    nx, ny, spp = 48, 48, 8
    _apply(sched, schedule, nx, ny)
    want, st0 = _render(ic.constant_room(nx, ny, "const"), nx, ny, spp)
    assert np.isfinite(want).all() and want.any()
    if schedule.startswith("chunks"):
        assert st0.chunks >= 2 and st0.lanes == 2, (st0.chunks, st0.lanes)
    if schedule == "tail":
        assert st0.finish_paths > 0
    if schedule.endswith("wavefront"):
        assert st0.finish_paths == 0 and st0.shade_hits > 0
    for mode in ("1x1", "5x3"):
        got, st = _render(ic.constant_room(nx, ny, mode), nx, ny, spp)
        ndiff = int((got.reshape(-1, 3) != want.reshape(-1, 3)).any(axis=1).sum())
        print("constant room, %s images, %s schedule: %d pixels differ; segments %d / %d"
              % (mode, schedule, ndiff, st.segments, st0.segments))
        assert np.array_equal(got, want)
        assert st.segments == st0.segments


def test_constant_images_equal_constant_textures_in_the_features(sched):
    nx, ny, spp = 48, 48, 8
    want = _features(ic.constant_room(nx, ny, "const"), nx, ny, spp)
    assert (want[:, 7] > 0).any()
    for mode in ("1x1", "5x3"):
        got = _features(ic.constant_room(nx, ny, mode), nx, ny, spp)
        assert np.array_equal(got, want), mode            # all 8 channels


# ------------------------------------------------------------------ 2. image rects == split rects
def test_image_rects_equal_split_rects_and_the_oracle(sched, oracle_mod):
    nx, ny, spp = 48, 48, 8
    allowance = spp * nx * ny // 1000                    # 18: the features test's allowance for exact ties
    img_scene, split_scene = ic.rect_room(nx, ny, False), ic.rect_room(nx, ny, True)
    a, sa = _render(img_scene, nx, ny, spp)
    b, sb = _render(split_scene, nx, ny, spp)
    differ = (a.reshape(-1, 3) != b.reshape(-1, 3)).any(axis=1)
    print("image rects vs split rects: %d of %d pixels differ (allowance %d, expected 0); segments %d / %d"
          % (differ.sum(), nx * ny, allowance, sa.segments, sb.segments))
    assert np.isfinite(a).all() and a.any()
    assert differ.sum() <= allowance
    if not differ.any():
        assert sa.segments == sb.segments
    # the whole path against the oracle, which holds the split twin
    ref, osegs = oracle_mod.build_scene(split_scene).render(nx, ny, 0, spp, SEED, nthreads=host_threads())
    keep = np.repeat(~differ, 3)
    rms, dmax, nbad, npx = parity._compare(a[keep], ref[keep], spp)
    print("image rects vs the oracle's split rects: rms=%.3e max=%.3e pixels>1e-9: %d/%d; segments gpu %d oracle %d"
          % (rms, dmax, nbad, npx, sa.segments, osegs))
    assert rms <= parity.RMS_TOL
    assert nbad <= max(2, npx // 200)
    # the wavefront kernels give the same image
    sched.set_option("tail_off", 1)
    c, sc_ = _render(img_scene, nx, ny, spp)
    assert np.array_equal(a, c) and sc_.segments == sa.segments


# ------------------------------------------------------------------ 3. sphere and moving-sphere u, v
def test_sphere_uv_albedo_matches_lookup_at_the_oracle_hit(sched, oracle_mod):
    nx, ny, spp = ic.SPHERE_FRAME
    allowance = spp * nx * ny // 1000                    # 4
    got = _features(ic.sphere_scene(nx, ny, True), nx, ny, spp)
    want = ic.sphere_expected_albedo()
    bad = (got[:, 0:3] != want).any(axis=1)
    print("sphere u, v: %d of %d pixels differ from lookup(sphere_uv(oracle hit)) (allowance %d)"
          % (bad.sum(), nx * ny, allowance))
    assert bad.sum() <= allowance
    # channels 3..7 (normal, t, hits) are those of the same spheres with constant textures
    plain = _features(ic.sphere_scene(nx, ny, False), nx, ny, spp)
    assert np.array_equal(got[:, 3:8], plain[:, 3:8])
    assert (got[:, 7] > 0).sum() > 100
    # and the render runs, on both schedules, to the same image
    a, _ = _render(ic.sphere_scene(nx, ny, True), nx, ny, spp)
    sched.set_option("tail_off", 1)
    b, _ = _render(ic.sphere_scene(nx, ny, True), nx, ny, spp)
    assert np.isfinite(a).all() and np.array_equal(a, b)


# ------------------------------------------------------------------ 4. cornell_image through Renderer
def test_cornell_image_renders_and_its_ppm_reads_back(sched, tmp_path):
    from rtamd.render import Renderer
    nx, ny, spp = 32, 32, 4
    scene = scenes.SCENES["cornell_image"](nx, ny)
    r = Renderer(nx, ny, seed=SEED)
    img = r.render(scene, spp)
    assert np.isfinite(r.raw_data).all() and img.any()
    # the floor shows its tiles: the image is not one colour there
    floor_rows = r.image.reshape(ny, nx, 3)[: ny // 4]
    assert len(np.unique(floor_rows.reshape(-1, 3), axis=0)) > 8
    path = str(tmp_path / "cornell_image.ppm")
    r.save_as_ppm(path)
    data, gx, gy = image.read_ppm(path)
    assert (gx, gy) == (nx, ny)
    assert np.array_equal(data.reshape(ny, nx, 3)[::-1], r.image.reshape(ny, nx, 3))
    # what was written is a texture
    from rtamd import scene as g
    assert g.make_image_texture(data, gx, gy).kind == "image"


# ------------------------------------------------------------------ the refusal that needs a committed scene
def test_committed_scene_takes_no_image(sched):
    nx, ny = 8, 8
    h = gpu.upload(scenes.test_scene(nx, ny))
    L = _lib.lib()
    out = ctypes.c_int(-7)
    px = (ctypes.c_uint8 * 12)()
    assert L.rt_add_texture_image(h, px, 2, 2, ctypes.byref(out)) != 0
    assert b"already committed" in L.rt_last_error() and out.value == -7
