"""Shared by test_features_host.py, test_denoise_host.py, test_gpu_features.py and test_gpu_denoise.py: the
oracle's first-hit features, built from the oracle's exports as they stand (trace_sample, hit_world,
tex_value, stream), and the oracle's moments for the denoiser's quality condition.  Every result is
computed once per session and returned read-only."""
import functools
import math

import numpy as np

from conftest import host_threads
from rtamd import scenes
from rtamd.scene import emit

SEED = 0x5EED0002
REF_SEED = 0x0DDBA11
#: the feature parity cases: scene name, nx, ny (passes 0 .. FEATURE_PASSES-1)
FEATURE_CASES = [("cornell", 48, 48), ("cover", 64, 36), ("cover_marble", 32, 18), ("curves_small", 48, 32),
                 ("klein", 32, 32), ("test_scene2", 32, 18), ("cover_horizon", 32, 18)]
FEATURE_PASSES = 4
#: the denoiser's quality cases (16 noisy passes against 1024 passes of another seed)
QUALITY_CASES = [("cornell", 48, 48), ("cover", 64, 36), ("cover_marble", 64, 36)]
QUALITY_PASSES, QUALITY_REF_PASSES = 16, 1024


@functools.lru_cache(maxsize=None)
def scene_of(name, nx, ny):
    if name == "cover_horizon":
        # the cover scene's objects seen from the side, with a lens: the library's cover camera looks down
        # from (0, 5, 5) and none of its rays reaches the sky, so this view supplies the gradient-sky misses
        from rtamd import vec as v
        from rtamd.camera import make_camera
        from rtamd.scene import make_scene
        base = scenes.random_scene(nx, ny)
        cam = make_camera(v.vec3(13, 2, 3), v.vec3(0, 0, 0), v.vec3(0, 1, 0), 20, nx / ny, 0.1, 10, 0, 1)
        return make_scene(base.obj_list, cam, base.sky_function)
    return scenes.SCENES[name](nx, ny)


def _recording_oracle():
    import oracle

    class RecordingOracle(oracle.OracleScene):
        """An OracleScene that remembers material id -> (kind, texture id) while a scene is emitted."""

        def __init__(self):
            super().__init__()
            self.materials = {}

        def _keep(self, mat, kind, tex):
            self.materials[mat] = (kind, tex)
            return mat

        def material_lambertian(self, tex):
            return self._keep(super().material_lambertian(tex), "lambertian", tex)

        def material_metal(self, tex, fuzz):
            return self._keep(super().material_metal(tex, fuzz), "metal", tex)

        def material_dielectric(self, r):
            return self._keep(super().material_dielectric(r), "dielectric", None)

        def material_diffuse_light(self, tex):
            return self._keep(super().material_diffuse_light(tex), "diffuse_light", tex)

    return RecordingOracle()


@functools.lru_cache(maxsize=None)
def oracle_scene(name, nx, ny):
    return emit(scene_of(name, nx, ny), _recording_oracle())


def camera_time(scene, seed, pix, smp):
    """The camera ray's time as camera_ray / cam:get-ray draw it: draws 0 and 1 are the jitter, then pairs
    (a, b) until (2a-1)^2 + (2b-1)^2 < 1, the next draw is the time."""
    import oracle
    slots = scene.camera.slots()
    t0, t1 = slots[22], slots[23]
    k, d = 2, oracle.stream(seed, pix, smp, 0, 64)
    while True:
        if k + 3 > len(d):
            d = oracle.stream(seed, pix, smp, 0, 2 * len(d))
        a, b = d[k], d[k + 1]
        k += 2
        px, py = a * 2.0 - 1.0, b * 2.0 - 1.0
        if px * px + py * py + 0.0 * 0.0 < 1.0:
            break
    return t0 + d[k] * (t1 - t0)


def sky_gradient(d):
    """sky-color (main.scm:91-95) of direction d, in the oracle's operation order."""
    r = 0.0
    r += d[0] * d[0]
    r += d[1] * d[1]
    r += d[2] * d[2]
    k = 1.0 / math.sqrt(r)
    t = 0.5 * (1.0 + d[1] * k)
    return tuple(1.0 * (1 - t) + c * t for c in (0.5, 0.7, 1.0))


def sample_features(name, nx, ny, j, smp, seed=SEED):
    """The eight feature values of pixel j's camera sample smp: albedo 3, normal 3, t, hit."""
    o = oracle_scene(name, nx, ny)
    y, x = divmod(j, nx)
    row = o.trace_sample(nx, ny, x, y, seed, smp, cap=1)[0]
    if row[6] == 0.0:                                          # miss: the sample's colour is the sky's
        return o.sample(nx, ny, x, y, seed, smp) + (0.0, 0.0, 0.0, 0.0, 0.0)
    rec = o.hit_world(row[0:3], row[3:6], camera_time(scene_of(name, nx, ny), seed, j, smp))
    assert rec is not None and rec[0] == row[7] and int(rec[7]) == int(row[11]), (name, j, smp, rec, row)
    kind, tex = o.materials[int(row[11])]
    albedo = (1.0, 1.0, 1.0) if kind == "dielectric" else o.tex_value(tex, row[8:11])
    return tuple(albedo) + tuple(rec[4:7]) + (row[7], 1.0)


@functools.lru_cache(maxsize=None)
def oracle_features(name, nx, ny, passes, seed=SEED):
    """(nx*ny, 8) running sums over passes 0 .. passes-1, each channel added in pass order."""
    feat = np.zeros((nx * ny, 8))
    for j in range(nx * ny):
        for smp in range(passes):
            feat[j] = feat[j] + np.array(sample_features(name, nx, ny, j, smp, seed))
    feat.setflags(write=False)
    return feat


@functools.lru_cache(maxsize=None)
def oracle_moments(name, nx, ny, passes, seed=SEED):
    """(S, Q): the oracle's running sums of passes 0 .. passes-1 and of their squares, in pass order."""
    o = oracle_scene(name, nx, ny)
    S = np.zeros(nx * ny * 3)
    Q = np.zeros(nx * ny * 3)
    for k in range(passes):
        a, _ = o.render(nx, ny, k, 1, seed, nthreads=host_threads())
        S = S + a
        Q = Q + a * a
    S.setflags(write=False)
    Q.setflags(write=False)
    return S, Q


@functools.lru_cache(maxsize=None)
def oracle_reference(name, nx, ny):
    """The mean of QUALITY_REF_PASSES oracle passes of another seed."""
    o = oracle_scene(name, nx, ny)
    a, _ = o.render(nx, ny, 0, QUALITY_REF_PASSES, REF_SEED, nthreads=host_threads())
    a = a / QUALITY_REF_PASSES
    a.setflags(write=False)
    return a


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a).ravel() - np.asarray(b).ravel()) ** 2)))
