"""First-hit feature buffers without a GPU: the ABI's refusals, the header, and self-checks of the oracle
features helper (tests/feature_cases.py) the GPU parity tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

import feature_cases as fc
from rtamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_announces_the_feature_buffers_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt)
    assert re.search(r"#define\s+RT_HAS_FEATURES\s+1\b", txt)
    assert re.search(r"#define\s+RT_FEATURE_DOUBLES\s+8\b", txt)
    assert _lib.RT_FEATURE_DOUBLES == 8
    assert {"rt_render_features", "rt_render_features_device"} <= set(_lib.EXPORTED)


def test_feature_entry_points_refuse_bad_arguments_without_gpu():
    """Null pointers, bad sizes and bad handles fail with a message before any device call."""
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.rt_render_features_device(424242, 4, 4, None, 0, 0, 1, 1, p, None) != 0
    assert b"invalid scene" in L.rt_last_error()
    assert L.rt_render_features(424242, 4, 4, 0, 1, 1, buf) != 0
    assert b"invalid scene" in L.rt_last_error()
    assert L.rt_render_features_device(424242, 4, 4, None, 0, 0, 1, 1, None, None) != 0
    assert b"null" in L.rt_last_error()
    assert L.rt_render_features(424242, 4, 4, 0, 1, 1, None) != 0
    assert b"null" in L.rt_last_error()
    assert L.rt_render_features_device(424242, 0, 4, None, 0, 0, 1, 1, p, None) != 0
    assert b"positive" in L.rt_last_error()
    assert L.rt_render_features(424242, 1 << 16, 1 << 16, 0, 1, 1, buf) != 0
    assert b"too large" in L.rt_last_error()
    assert L.rt_render_features_device(424242, 4, 4, None, 0, -1, 1, 1, p, None) != 0
    assert b"spp" in L.rt_last_error()
    assert L.rt_render_features(424242, 4, 4, 0, -1, 1, buf) != 0
    assert b"spp" in L.rt_last_error()
    # a list longer than the frame, or of negative length
    assert L.rt_render_features_device(424242, 4, 4, p, 17, 0, 1, 1, p, None) != 0
    assert b"pixel list length" in L.rt_last_error()
    assert L.rt_render_features_device(424242, 4, 4, p, -1, 0, 1, 1, p, None) != 0
    assert b"pixel list length" in L.rt_last_error()


@pytest.mark.parametrize("name,nx,ny", fc.FEATURE_CASES)
def test_oracle_features_are_consistent(name, nx, ny, oracle_mod):
    """hits <= passes; a miss adds nothing to normal and t; unit normals (spheres, rects) sum to at most
    hits in length."""
    f = fc.oracle_features(name, nx, ny, fc.FEATURE_PASSES)
    hits = f[:, 7]
    assert np.isfinite(f).all()
    assert ((hits >= 0) & (hits <= fc.FEATURE_PASSES) & (hits == np.round(hits))).all()
    miss = hits == 0
    assert (f[miss, 3:7] == 0).all()
    assert (f[~miss, 6] > 0).all()
    if name in ("cornell", "cover", "cover_marble", "test_scene2", "cover_horizon"):
        assert (np.sqrt((f[:, 3:6] ** 2).sum(axis=1)) <= hits + 1e-9).all()
    if name == "curves_small":
        assert miss.any() and (~miss).any()                   # both branches of the helper are exercised


def test_cover_miss_samples_carry_the_sky_gradient(oracle_mod):
    """A camera sample that misses everything has the gradient of its own direction as albedo, and nothing
    else.  The cover scene's own camera looks down from (0, 5, 5) and every one of its rays hits the ground
    (asserted), so the misses come from the same objects seen from the side (cover_horizon)."""
    o = fc.oracle_scene("cover", 64, 36)
    assert all(o.trace_sample(64, 36, x, 35, fc.SEED, 0, cap=1)[0][6] == 1.0 for x in range(64))
    name, nx, ny = "cover_horizon", 32, 18
    o = fc.oracle_scene(name, nx, ny)
    found = 0
    for j in range(nx * ny):
        y, x = divmod(j, nx)
        row = o.trace_sample(nx, ny, x, y, fc.SEED, 0, cap=1)[0]
        v = fc.sample_features(name, nx, ny, j, 0)
        if row[6] == 0.0:
            found += 1
            assert v[:3] == fc.sky_gradient(row[3:6]) and v[3:] == (0.0,) * 5
            assert all(0.5 <= c <= 1.0 for c in v[:3])
        else:
            assert v[7] == 1.0
    print("%s %dx%d: %d pass-0 samples miss" % (name, nx, ny, found))
    assert 0 < found < nx * ny


def test_camera_time_follows_the_draw_order(oracle_mod):
    """The time draw comes after the jitter pair and the accepted disk pair: for the cover scene's camera
    (shutter 0 .. 1) the time is that draw itself."""
    sc = fc.scene_of("cover", 64, 36)
    assert tuple(sc.camera.slots()[22:24]) == (0.0, 1.0)
    import oracle
    for pix, smp in ((0, 0), (17, 3), (2303, 1)):
        d = oracle.stream(fc.SEED, pix, smp, 0, 40)
        k = 2
        while True:
            a, b = d[k] * 2.0 - 1.0, d[k + 1] * 2.0 - 1.0
            if a * a + b * b < 1.0:
                break
            k += 2
        assert fc.camera_time(sc, fc.SEED, pix, smp) == d[k + 2]
