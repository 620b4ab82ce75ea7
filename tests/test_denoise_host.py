"""The denoiser without a GPU: the ABI's refusals, the rule's properties on synthetic inputs
(rtamd.denoise.atrous, the NumPy restatement of include/rt.h's rule), and the quality condition the
feature is for: on the oracle's own 16 passes the filtered image is closer to a 1024-pass reference
than the noisy one."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import feature_cases as fc
from rtamd import _lib, denoise, gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = denoise.DEFAULTS


def ulps(a, b):
    """|a - b| in units of the spacing of doubles at |b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def synthetic(nx, ny, colour, albedo=(1.0, 1.0, 1.0), normal=(0.0, 0.0, 1.0), z=1.0, n=4, m=2):
    """Sums of n samples that all equal `colour` (so Q - S*S/n is exactly 0) and of m feature passes that all
    hit; every argument may be a scalar / triple or a per-pixel (ny, nx[, 3]) array."""
    c = np.broadcast_to(np.asarray(colour, dtype=np.float64), (ny, nx, 3))
    S = c * float(n)
    Q = (S * S) / float(n)
    feat = np.zeros((ny, nx, 8))
    feat[..., 0:3] = np.broadcast_to(np.asarray(albedo, dtype=np.float64), (ny, nx, 3)) * m
    feat[..., 3:6] = np.broadcast_to(np.asarray(normal, dtype=np.float64), (ny, nx, 3)) * m
    feat[..., 6] = np.broadcast_to(np.asarray(z, dtype=np.float64), (ny, nx)) * m
    feat[..., 7] = m
    return S.reshape(-1).copy(), Q.reshape(-1).copy(), feat.reshape(-1, 8).copy(), n, m


def atrous_scalar(S, Q, count, sample_count, feat, feat_count, nx, ny, iterations, normal_squarings, sigma_z, sigma_l,
                  albedo_floor):
    """include/rt.h's rule pixel by pixel in plain Python floats: an independent restatement that
    rtamd.denoise.atrous (array slices) must match bit for bit."""
    kern = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
    S = np.asarray(S).reshape(-1, 3)
    f = np.asarray(feat).reshape(-1, 8)
    m = float(feat_count)
    U, V, DEN, G = [], [], [], []
    for j in range(nx * ny):
        n = float(sample_count if count is None else count[j])
        den = [f[j, k] / m if f[j, k] / m > albedo_floor else albedo_floor for k in range(3)]
        u = [(0.0 if n == 0.0 else S[j, k] / n) / den[k] for k in range(3)]
        v = 0.0
        if Q is not None and n >= 2.0:
            e = []
            for k in range(3):
                d = float(np.asarray(Q).reshape(-1, 3)[j, k]) - (S[j, k] * S[j, k]) / n
                e.append(((0.0 if d < 0.0 else d) / (n * (n - 1.0))) / (den[k] * den[k]))
            v = (e[0] + e[1]) + e[2]
        U.append([float(x) for x in u]); V.append(float(v)); DEN.append(den)
        G.append([float(f[j, 3] / m), float(f[j, 4] / m), float(f[j, 5] / m), float(f[j, 6] / m), float(f[j, 7] / m)])
    ok = lambda j: all(math.isfinite(x) for x in U[j]) and math.isfinite(V[j])
    for i in range(iterations):
        s = 1 << i
        U2, V2 = [list(u) for u in U], list(V)
        for y in range(ny):
            for x in range(nx):
                p = y * nx + x
                if not ok(p):
                    continue
                lp = (U[p][0] + U[p][1]) + U[p][2]
                W, A, B = 0.0, [0.0, 0.0, 0.0], 0.0
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        xx, yy = x + dx * s, y + dy * s
                        if not (0 <= xx < nx and 0 <= yy < ny):
                            continue
                        q = yy * nx + xx
                        hk = kern[dy + 2] * kern[dx + 2]
                        if dx == 0 and dy == 0:
                            w = hk
                        else:
                            if not ok(q):
                                continue
                            if G[p][4] == 0.0 and G[q][4] == 0.0:
                                wn = 1.0
                            else:
                                g = (G[p][0] * G[q][0] + G[p][1] * G[q][1]) + G[p][2] * G[q][2]
                                wn = g if g > 0.0 else 0.0
                                for _ in range(normal_squarings):
                                    wn = wn * wn
                            zm = G[p][3] if G[p][3] > G[q][3] else G[q][3]
                            wz = float(np.exp(-(abs(G[p][3] - G[q][3]) / (sigma_z * zm + 1e-300))))
                            wl = 1.0
                            if Q is not None:
                                lq = (U[q][0] + U[q][1]) + U[q][2]
                                wl = float(np.exp(-(abs(lp - lq) / (sigma_l * math.sqrt(V[p]) + 1e-10))))
                            w = ((hk * wn) * wz) * wl
                        W = W + w
                        for k in range(3):
                            A[k] = A[k] + w * U[q][k]
                        B = B + (w * w) * V[q]
                U2[p] = [A[k] / W for k in range(3)]
                V2[p] = B / (W * W)
        U, V = U2, V2
    return np.array([[U[j][k] * DEN[j][k] for k in range(3)] for j in range(nx * ny)]).reshape(-1)


# ------------------------------------------------------------------ the ABI
def test_header_announces_the_denoiser():
    txt = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+7\b", txt)
    assert re.search(r"#define\s+RT_HAS_DENOISE\s+1\b", txt)
    assert {"rt_denoise", "rt_denoise_device"} <= set(_lib.EXPORTED)
    assert ctypes.sizeof(_lib.RtDenoise) == 32


def _call(entry, ctx, nx, ny, p, accum, accum2, count, n, feat, m, out):
    L = _lib.lib()
    if entry == "rt_denoise_device":
        return L.rt_denoise_device(ctx, nx, ny, p, accum, accum2, count, n, feat, m, out, None)
    dp = ctypes.POINTER(ctypes.c_double)
    cast = lambda v, t: None if v is None else ctypes.cast(v, t)
    return L.rt_denoise(ctx, nx, ny, p, cast(accum, dp), cast(accum2, dp), cast(count, ctypes.POINTER(ctypes.c_uint32)), n,
                        cast(feat, dp), m, cast(out, dp))


@pytest.mark.parametrize("entry", ["rt_denoise_device", "rt_denoise"])
def test_denoise_refuses_bad_arguments_without_gpu(entry):
    """Bad handles, null pointers and each bad parameter fail with a message before any device call."""
    L = _lib.lib()
    a, f, o = (ctypes.c_double * 48)(), (ctypes.c_double * 128)(), (ctypes.c_double * 48)()
    pa, pf, po = (ctypes.cast(x, ctypes.c_void_p) for x in (a, f, o))
    good = gpu.denoise_params()
    ref = ctypes.byref
    assert _call(entry, 424242, 4, 4, ref(good), pa, None, None, 4, pf, 4, po) != 0
    assert b"invalid context" in L.rt_last_error()
    for bad, word in ((dict(iterations=0), b"iterations"), (dict(iterations=13), b"iterations"),
                      (dict(normal_squarings=17), b"normal_squarings"),
                      (dict(sigma_z=0.0), b"sigma_z"), (dict(sigma_z=-1.0), b"sigma_z"), (dict(sigma_z=float("nan")), b"sigma_z"),
                      (dict(sigma_l=0.0), b"sigma_l"), (dict(sigma_l=float("inf")), b"sigma_l"),
                      (dict(albedo_floor=0.0), b"albedo_floor"), (dict(albedo_floor=float("nan")), b"albedo_floor")):
        p = gpu.denoise_params(**bad)
        assert _call(entry, 424242, 4, 4, ref(p), pa, None, None, 4, pf, 4, po) != 0, bad
        assert word in L.rt_last_error(), (bad, L.rt_last_error())
        with pytest.raises(ValueError):
            denoise.check_params(**dict(D, **bad))
    assert _call(entry, 424242, 4, 4, ref(good), pa, None, None, 4, pf, 0, po) != 0
    assert b"feat_count" in L.rt_last_error()
    assert _call(entry, 424242, 4, 4, None, pa, None, None, 4, pf, 4, po) != 0
    assert b"null" in L.rt_last_error()
    for args in ((None, pf, po), (pa, None, po), (pa, pf, None)):
        assert _call(entry, 424242, 4, 4, ref(good), args[0], None, None, 4, args[1], 4, args[2]) != 0
        assert b"null" in L.rt_last_error()
    assert _call(entry, 424242, 0, 4, ref(good), pa, None, None, 4, pf, 4, po) != 0
    assert b"positive" in L.rt_last_error()
    assert _call(entry, 424242, 4, 4, ref(good), pa, None, None, 4, pf, 4, pa) != 0
    assert b"alias" in L.rt_last_error()
    denoise.check_params(**D)


# --------------------------------------------------- the rule on synthetic inputs
def test_atrous_matches_the_scalar_restatement_bit_for_bit():
    """The array-slice implementation against the header's rule pixel by pixel: a 7x5 frame with random
    sums, features, counts and a non-finite pixel, and the 3x2 frame whose taps mostly fall outside."""
    rng = np.random.default_rng(5)
    for nx, ny, iters in ((7, 5, 3), (3, 2, 5), (1, 1, 2)):
        npx = nx * ny
        x = rng.random((6, npx, 3))
        S, Q = x.sum(axis=0), (x * x).sum(axis=0)
        count = rng.integers(0, 7, npx).astype(np.uint32)
        feat = np.zeros((npx, 8))
        feat[:, 0:3] = rng.random((npx, 3)) * 3
        feat[:, 3:6] = rng.normal(size=(npx, 3))
        feat[:, 7] = rng.integers(0, 4, npx)
        feat[:, 6] = rng.random(npx) * 10 * feat[:, 7]
        if npx > 4:
            S[3, 1] = np.nan
        for q, c in ((Q, count), (None, None), (Q, None)):
            got = denoise.atrous(S.reshape(-1), None if q is None else q.reshape(-1), c, 6, feat, 3, nx, ny,
                                 **dict(D, iterations=iters))
            want = atrous_scalar(S.reshape(-1), q, c, 6, feat, 3, nx, ny, iters, D["normal_squarings"], D["sigma_z"],
                                 D["sigma_l"], D["albedo_floor"])
            assert np.array_equal(got, want, equal_nan=True), (nx, ny, np.abs(got - want).max())


def test_uniform_frame_is_unchanged():
    """Uniform features, a constant image and zero variance: every weight is hk, so the output is the input
    mean to within 4 ulp (the divisions and the weighted mean round)."""
    nx, ny = 21, 13
    colour = (0.3, 0.6, 0.9)
    S, Q, feat, n, m = synthetic(nx, ny, colour, albedo=(0.7, 0.5, 0.2))
    out = denoise.atrous(S, Q, None, n, feat, m, nx, ny).reshape(-1, 3)
    u = ulps(out, np.broadcast_to(colour, out.shape))
    print("uniform frame: max deviation %.2f ulp" % u.max())
    assert u.max() <= 4.0


def test_orthogonal_normals_do_not_mix():
    """Two half-frames with orthogonal normals and different constants (accum2 NULL, so only wn separates
    them): the cross weights are exactly 0 and neither side moves (the uniform frame's 4 ulp)."""
    nx, ny = 20, 9
    left = np.arange(nx) < nx // 2
    colour = np.where(left[None, :, None], 0.2, 0.8) * np.ones((ny, nx, 3))
    normal = np.where(left[None, :, None], (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)) * np.ones((ny, nx, 3))
    S, _, feat, n, m = synthetic(nx, ny, colour, normal=normal)
    out = denoise.atrous(S, None, None, n, feat, m, nx, ny).reshape(ny, nx, 3)
    u = ulps(out, colour)
    print("orthogonal normals: max deviation %.2f ulp" % u.max())
    assert u.max() <= 4.0


@pytest.mark.parametrize("sigma_z", [0.1, 0.01])
def test_depth_edge_leaks_at_most_its_weight(sigma_z):
    """Two half-frames that differ only in z by a factor of 10 (accum2 NULL): a tap across the edge has
    wz = exp(-|z_p - z_q| / (sigma_z max(z_p, z_q))) = exp(-0.9 / sigma_z) — exp(-9) at the default sigma_z
    = 0.1, exp(-90) = exp(-9 / 0.1) at 0.01.  Of a pixel's kernel row at most 5/16 lies across the edge and at
    least 11/16 on its own side, and values stay between the two constants, so one iteration moves a pixel
    by at most (5/11) wz |B - A| and `iterations` of them by at most iterations times that; plus the uniform
    frame's 4 ulp of rounding."""
    nx, ny = 20, 9
    A, B = 0.2, 0.8
    left = np.arange(nx) < nx // 2
    colour = np.where(left[None, :, None], A, B) * np.ones((ny, nx, 3))
    z = np.where(left[None, :], 1.0, 10.0) * np.ones((ny, nx))
    S, _, feat, n, m = synthetic(nx, ny, colour, z=z)
    out = denoise.atrous(S, None, None, n, feat, m, nx, ny, **dict(D, sigma_z=sigma_z)).reshape(ny, nx, 3)
    bound = D["iterations"] * (5.0 / 11.0) * math.exp(-0.9 / sigma_z) * (B - A) + 4 * np.spacing(B)
    moved = np.abs(out - colour).max()
    print("depth edge, sigma_z %g: moved %.3e, bound %.3e" % (sigma_z, moved, bound))
    assert moved <= bound
    if sigma_z == 0.1:
        assert moved > 0.0                                    # the leak is there, and small


def test_non_finite_pixels_pass_through_and_are_never_taps():
    """A NaN sum and an infinite second moment: those pixels come out as they went in (u * den), and every
    other pixel of the constant frame stays within the uniform frame's 4 ulp — no tap used them."""
    nx, ny = 15, 11
    colour = (0.3, 0.6, 0.9)
    S, Q, feat, n, m = synthetic(nx, ny, colour)
    S = S.reshape(-1, 3)
    Q = Q.reshape(-1, 3)
    a, b = 5 * nx + 7, 2 * nx + 3
    S[a, 1] = np.nan
    Q[b, 0] = np.inf
    out = denoise.atrous(S.reshape(-1), Q.reshape(-1), None, n, feat, m, nx, ny).reshape(-1, 3)
    assert np.isnan(out[a, 1]) and ulps(out[a, [0, 2]], np.array(colour)[[0, 2]]).max() <= 1.0
    assert ulps(out[b], colour).max() <= 1.0
    rest = np.ones(nx * ny, dtype=bool)
    rest[[a, b]] = False
    assert np.isfinite(out[rest]).all()
    assert ulps(out[rest], np.broadcast_to(colour, out[rest].shape)).max() <= 4.0


def test_taps_outside_a_tiny_frame_are_skipped():
    """A 3x2 frame with 5 iterations (steps up to 16 reach far outside): finite, within the inputs' range, and
    from step 4 on only the centre tap is left, so iterations 3..5 change nothing beyond their rounding."""
    nx, ny = 3, 2
    rng = np.random.default_rng(11)
    colour = rng.random((ny, nx, 3))
    S, Q, feat, n, m = synthetic(nx, ny, colour)
    out5 = denoise.atrous(S, Q, None, n, feat, m, nx, ny, **dict(D, iterations=5))
    out2 = denoise.atrous(S, Q, None, n, feat, m, nx, ny, **dict(D, iterations=2))
    assert np.isfinite(out5).all()
    assert out5.min() >= colour.min() - 1e-15 and out5.max() <= colour.max() + 1e-15
    assert ulps(out5, out2).max() <= 8.0


# --------------------------------------------------------- what the feature is for
@pytest.mark.parametrize("name,nx,ny", fc.QUALITY_CASES)
def test_denoised_is_closer_to_the_reference_than_noisy(name, nx, ny, oracle_mod):
    """The oracle's first 16 passes (S, Q) and the oracle helper's 16-pass features through atrous at the
    defaults, against 1024 oracle passes of another seed: RMSE(denoised) < RMSE(noisy)."""
    S, Q = fc.oracle_moments(name, nx, ny, fc.QUALITY_PASSES)
    feat = fc.oracle_features(name, nx, ny, fc.QUALITY_PASSES)
    ref = fc.oracle_reference(name, nx, ny)
    den = denoise.atrous(S, Q, None, fc.QUALITY_PASSES, feat, fc.QUALITY_PASSES, nx, ny)
    noisy, filt = fc.rmse(S / fc.QUALITY_PASSES, ref), fc.rmse(den, ref)
    print("%s %dx%d: RMSE noisy %.4f denoised %.4f" % (name, nx, ny, noisy, filt))
    assert np.isfinite(den).all()
    assert filt < noisy
