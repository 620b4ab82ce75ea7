"""Adaptive sampling without a GPU: the per-count resolve, the stop rule's NumPy restatement, the new
entry points' argument checks, and the replay of the rounds over the oracle's per-pass colours that
licenses the exact comparisons of test_gpu_adaptive.py."""
import ctypes

import numpy as np
import pytest

import adaptive_cases as ac
from rtamd import _lib, adaptive, gpu

BAD = 424242                    # no such context / scene


# ------------------------------------------------------------ rt_resolve_u8_counts
def test_resolve_counts_matches_numpy():
    nx, ny = 7, 5
    rs = np.random.RandomState(11)
    count = rs.choice(np.array([0, 1, 4, 1000], dtype=np.uint32), size=nx * ny)
    count[:4] = [0, 1, 4, 1000]                                   # every value occurs
    acc = rs.uniform(0, 5, size=nx * ny * 3) * np.repeat(np.maximum(count, 1), 3)
    acc[3:6] = [0.0, 1.0, 1.0000001]                              # count 1: black, exactly 1, just above
    want = np.zeros(nx * ny * 3, dtype=np.uint8)
    for i in range(nx * ny * 3):
        n = int(count[i // 3])
        if n:
            want[i] = int(np.floor(255.99 * min(1.0, np.sqrt(acc[i] / float(n)))))
    got = gpu.resolve_u8_counts(acc, count, nx, ny)
    assert np.array_equal(got, want)
    assert not got.reshape(-1, 3)[count == 0].any()


@pytest.mark.parametrize("n", [1, 4, 1000])
def test_resolve_equal_counts_is_the_plain_resolve(n):
    nx, ny = 7, 5
    acc = np.random.RandomState(12).uniform(0, 1.3 * n, size=nx * ny * 3)
    count = np.full(nx * ny, n, dtype=np.uint32)
    assert np.array_equal(gpu.resolve_u8_counts(acc, count, nx, ny), gpu.resolve_u8(acc, nx, ny, n))


# ------------------------------------------------------------ adaptive.converged, by hand
def _moments(samples):
    """In-order sums of per-channel samples (k, 3) as the kernels form them."""
    S = np.zeros(3)
    Q = np.zeros(3)
    for x in np.asarray(samples, dtype=np.float64):
        S = S + x
        Q = Q + x * x
    return S, Q, len(samples)


def test_converged_zero_pixel():
    S, Q, n = _moments(np.zeros((4, 3)))
    assert adaptive.converged(S, Q, n, 0.1, 0.05)
    assert adaptive.converged(S, Q, n, 0.0, 0.05)                # 0 <= 0
    assert adaptive.relative_error(S, Q, n, 0.05) == 0.0


def test_converged_two_samples():
    # per channel 0.25, 0.75: d = 0.625 - 1/2 = 0.125, v = 0.125 / 2, e2 = 0.1875, m = 1.5 -> tol >= sqrt(0.1875)/1.5
    S, Q, n = _moments([[0.25] * 3, [0.75] * 3])
    assert n == 2 and adaptive.relative_error(S, Q, n, 0.05) == np.sqrt(0.1875) / 1.5
    assert adaptive.converged(S, Q, n, 0.29, 0.05)
    assert not adaptive.converged(S, Q, n, 0.28, 0.05)
    # one sample, or none: 0 / 0, never converged
    assert not adaptive.converged(S, Q, 1, 1e6, 0.05)
    assert not adaptive.converged(np.zeros(3), np.zeros(3), 0, 1e6, 0.05)


def test_converged_clamps_a_rounding_negative_variance():
    S, Q, n = _moments([[0.7, 0.3, 0.7]] * 7)                   # constant samples: the true variance is 0
    d = Q - (S * S) / n
    assert (d < 0).all() and (np.abs(d) < 1e-14).all()          # ... and rounding drives it below
    assert adaptive.relative_error(S, Q, n, 0.05) == 0.0
    assert adaptive.converged(S, Q, n, 0.0, 0.05)


def test_converged_mean_below_floor():
    # per channel 0, 0, 0, 0.04: e2 = 3e-4, m = 0.03; tol 0.5: (0.5 * 0.05)^2 = 6.25e-4 but (0.5 * 0.03)^2 = 2.25e-4
    S, Q, n = _moments([[0.0] * 3] * 3 + [[0.04] * 3])
    assert adaptive.converged(S, Q, n, 0.5, 0.05)
    assert not adaptive.converged(S, Q, n, 0.5, 0.0)
    assert not adaptive.converged(S, Q, n, 0.5, 0.02)


def test_converged_tol_zero_needs_zero_variance():
    S, Q, n = _moments([[0.5] * 3] * 4)                         # exact: Q = 1, S*S/n = 1
    assert adaptive.converged(S, Q, n, 0.0, 0.05)
    S, Q, n = _moments([[0.5] * 3] * 3 + [[0.5, 0.5, 0.5000001]])
    assert not adaptive.converged(S, Q, n, 0.0, 0.05)


def test_converged_nan_moments_never():
    S, Q, n = _moments([[0.5] * 3] * 4)
    nan = float("nan")
    for Sx, Qx in ((S * [1, nan, 1], Q), (S, Q * [nan, 1, 1]), (S * nan, Q * nan), (S, Q + [0, 0, float("inf")])):
        assert not adaptive.converged(Sx, Qx, n, 1e6, 0.05)
        assert not adaptive.converged(Sx, Qx, n, 0.0, 0.05)


def test_converged_broadcasts_over_pixels():
    rs = np.random.RandomState(5)
    x = rs.uniform(0, 1, size=(6, 50, 3))
    S = np.zeros((50, 3))
    Q = np.zeros((50, 3))
    for k in range(6):
        S = S + x[k]
        Q = Q + x[k] * x[k]
    got = adaptive.converged(S, Q, np.full(50, 6, dtype=np.uint32), 0.15, 0.05)
    want = [bool(adaptive.converged(S[j], Q[j], 6, 0.15, 0.05)) for j in range(50)]
    assert got.tolist() == want and 0 < sum(want) < 50


# ------------------------------------------------------------ argument and handle checks
def _err(status):
    assert status != 0
    return _lib.lib().rt_last_error()


def _params(min_spp=4, max_spp=24, batch_spp=4, tol=0.2, floor=0.05):
    return _lib.RtAdaptive(min_spp, max_spp, batch_spp, 0, tol, floor)


P1 = ctypes.c_void_p(16)        # a non-null pointer no check may follow


def test_adaptive_entry_points_refuse_bad_handles_without_gpu():
    L = _lib.lib()
    m, cap = ctypes.c_int64(0), ctypes.c_int64(0)
    res = _lib.RtAdaptiveResult()
    host = np.zeros(4 * 4 * 3)
    cnt = np.zeros(4 * 4, dtype=np.uint32)
    dp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cp = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert b"invalid scene" in _err(L.rt_render_pixels_device(BAD, 4, 4, P1, 3, 0, 1, 1, P1, P1, P1, None))
    assert b"invalid scene" in _err(L.rt_render_pixels_device(BAD, 4, 4, P1, 0, 0, 1, 1, P1, None, None, None))
    assert b"invalid context" in _err(L.rt_adaptive_select_device(BAD, None, 3, P1, P1, P1, 0.1, 0.05, 8, P1,
                                                                  ctypes.byref(m), ctypes.byref(cap), None))
    assert b"invalid scene" in _err(L.rt_render_adaptive_device(BAD, 4, 4, ctypes.byref(_params()), 1, P1, P1, P1, None,
                                                                ctypes.byref(res)))
    assert b"invalid scene" in _err(L.rt_render_adaptive(BAD, 4, 4, ctypes.byref(_params()), 1, dp, dp, cp,
                                                         ctypes.byref(res)))
    assert b"invalid context" in _err(L.rt_resolve_u8_counts_device(BAD, P1, P1, 4, 4, P1, None))
    assert not host.any() and not cnt.any()


def test_render_pixels_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    f = L.rt_render_pixels_device
    assert b"null pixel list" in _err(f(BAD, 4, 4, None, 3, 0, 1, 1, P1, P1, P1, None))
    assert b"null accum" in _err(f(BAD, 4, 4, P1, 3, 0, 1, 1, None, P1, P1, None))
    assert b"list length -1" in _err(f(BAD, 4, 4, P1, -1, 0, 1, 1, P1, P1, P1, None))
    assert b"list length 17" in _err(f(BAD, 4, 4, P1, 17, 0, 1, 1, P1, P1, P1, None))
    assert b"positive" in _err(f(BAD, 0, 4, P1, 0, 0, 1, 1, P1, P1, P1, None))
    assert b"too large" in _err(f(BAD, 1 << 16, 1 << 16, P1, 3, 0, 1, 1, P1, P1, P1, None))
    assert b"spp_begin" in _err(f(BAD, 4, 4, P1, 3, -1, 1, 1, P1, P1, P1, None))
    assert b"spp_begin" in _err(f(BAD, 4, 4, P1, 3, 0, -1, 1, P1, P1, P1, None))


def test_select_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    m, cap = ctypes.c_int64(7), ctypes.c_int64(7)
    rm, rc = ctypes.byref(m), ctypes.byref(cap)

    def f(pix_in=None, n=3, a=P1, a2=P1, c=P1, tol=0.1, floor=0.05, out=P1, om=rm, oc=rc):
        return L.rt_adaptive_select_device(BAD, pix_in, n, a, a2, c, tol, floor, 8, out, om, oc, None)
    for kw in (dict(a=None), dict(a2=None), dict(c=None), dict(out=None), dict(om=None), dict(oc=None)):
        assert b"null" in _err(f(**kw))
    assert b"list length" in _err(f(n=-1))
    assert b"list length" in _err(f(n=1 << 31))
    for bad in (-0.1, float("nan"), float("inf")):
        assert b"tol" in _err(f(tol=bad))
        assert b"floor" in _err(f(floor=bad))
    assert b"pix_out" in _err(f(pix_in=P1, out=P1))
    assert m.value == 7 and cap.value == 7


@pytest.mark.parametrize("entry", ["rt_render_adaptive_device", "rt_render_adaptive"])
def test_adaptive_render_refuses_bad_parameters_without_gpu(entry):
    L = _lib.lib()
    res = _lib.RtAdaptiveResult()
    host = np.zeros(4 * 4 * 3)
    cnt = np.zeros(4 * 4, dtype=np.uint32)
    dp = host.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cp = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))

    def f(p, nx=4, ny=4, a=True, a2=True, c=True):
        pp = ctypes.byref(p) if p is not None else None
        if entry == "rt_render_adaptive_device":
            return L.rt_render_adaptive_device(BAD, nx, ny, pp, 1, P1 if a else None, P1 if a2 else None,
                                               P1 if c else None, None, ctypes.byref(res))
        return L.rt_render_adaptive(BAD, nx, ny, pp, 1, dp if a else None, dp if a2 else None, cp if c else None,
                                    ctypes.byref(res))
    assert b"null" in _err(f(None))
    for kw in (dict(a=False), dict(a2=False), dict(c=False)):
        assert b"null" in _err(f(_params(), **kw))
    assert b"min_spp" in _err(f(_params(min_spp=1)))
    assert b"min_spp" in _err(f(_params(min_spp=0)))
    assert b"max_spp" in _err(f(_params(min_spp=8, max_spp=7)))
    assert b"batch_spp" in _err(f(_params(batch_spp=0)))
    for bad in (-1e-9, float("nan"), float("inf")):
        assert b"tol" in _err(f(_params(tol=bad)))
        assert b"floor" in _err(f(_params(floor=bad)))
    assert b"positive" in _err(f(_params(), nx=0))
    assert b"too large" in _err(f(_params(), nx=1 << 16, ny=1 << 16))
    assert not host.any() and not cnt.any()


def test_resolve_counts_refuses_null_buffers():
    L = _lib.lib()
    acc = np.zeros(3)
    cnt = np.ones(1, dtype=np.uint32)
    out = np.zeros(3, dtype=np.uint8)
    dp = acc.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cp = cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert b"null" in _err(L.rt_resolve_u8_counts(None, cp, 1, 1, op))
    assert b"null" in _err(L.rt_resolve_u8_counts(dp, None, 1, 1, op))
    assert b"null" in _err(L.rt_resolve_u8_counts(dp, cp, 1, 1, None))
    assert b"positive" in _err(L.rt_resolve_u8_counts(dp, cp, 0, 1, op))
    assert b"null" in _err(L.rt_resolve_u8_counts_device(BAD, None, P1, 1, 1, P1, None))
    with pytest.raises(ValueError):
        gpu.resolve_u8_counts(np.zeros(6), np.ones(1, dtype=np.uint32), 1, 1)


def test_header_announces_the_feature_and_keeps_the_abi_version():
    import os
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt.h")).read()
    assert "#define RT_HAS_ADAPTIVE 1" in txt and "#define RT_ABI_VERSION 7" in txt
    assert ctypes.sizeof(_lib.RtAdaptive) == 32 and ctypes.sizeof(_lib.RtAdaptiveResult) == 48


# ------------------------------------------------------------ the oracle's replay of the stop rule
@pytest.mark.parametrize("name,nx,ny", ac.CASES)
def test_oracle_replay_spreads_counts_and_avoids_the_threshold(name, nx, ny, oracle_mod):
    """The reference's own colours through the rounds: every count 4, 8, .., 24 occurs, and no pixel's e2
    lies within 1e-9 r^2 of r^2 in any round — so an ulp of difference between the device's sin / cos / pow
    and the C library's cannot flip a verdict, and the GPU tests may compare counts exactly."""
    passes = ac.oracle_passes(name, nx, ny)
    npix = nx * ny
    S = np.zeros((npix, 3))
    Q = np.zeros((npix, 3))
    count = np.zeros(npix, dtype=np.uint32)
    active = np.ones(npix, dtype=bool)
    done = 0
    near = 0
    while active.any() and done < ac.MAX_SPP:
        step = ac.MIN_SPP if done == 0 else min(ac.BATCH_SPP, ac.MAX_SPP - done)
        for k in range(done, done + step):
            x = passes[k][active]
            S[active] = S[active] + x
            Q[active] = Q[active] + x * x
        count[active] += np.uint32(step)
        done += step
        e2, b = adaptive._terms(S[active], Q[active], count[active], ac.FLOOR)
        r2 = (ac.TOL * b) * (ac.TOL * b)
        near += int((np.abs(e2 - r2) <= 1e-9 * r2).sum())
        active[active] = ~(e2 <= r2)
    hist = [int((count == c).sum()) for c in range(ac.MIN_SPP, ac.MAX_SPP + 1, ac.BATCH_SPP)]
    print(name, hist, "near the threshold:", near)
    assert sum(hist) == npix and all(h > 0 for h in hist)
    assert near == 0
    # adaptive.replay is the same loop
    S2, Q2, count2, rounds, capped = adaptive.replay(passes, ac.MIN_SPP, ac.MAX_SPP, ac.BATCH_SPP, ac.TOL, ac.FLOOR)
    assert np.array_equal(count2, count) and np.array_equal(S2, S) and np.array_equal(Q2, Q)
    assert rounds == 6 and capped == int(active.sum())
