"""The kernels' lean f64 helpers (scheme-raytrace_amd/csrc/rt_f64.h, through rt_f64_probe) against numpy's
sqrt and 1.0 / x on the host, bit for bit: both are the correctly rounded IEEE operations and know nothing
of the code under test.  sqrt_mid / rcp_mid must give those bits for every input (the window's core inside
[2^-256, 2^256), the plain operation outside); sqrt_core / rcp_core are asked only inside the window and
on the random draws' grid (2k+1) 2^-53, where the render path calls them unguarded."""
import numpy as np
import pytest

from rtamd import gpu

pytestmark = pytest.mark.gpu

BIAS = 1023
LO, HI = BIAS - 256, BIAS + 256          # biased exponents: the window is LO <= e < HI
MANT = (1 << 52) - 1
PATTERNS = np.array([0, 1, MANT, MANT - 1, 1 << 51], dtype=np.uint64)


def _f(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def _with_exponents(exps, mants):
    e = np.asarray(exps, dtype=np.uint64)[:, None] << np.uint64(52)
    return _f((e | np.asarray(mants, dtype=np.uint64)[None, :]).ravel())


def _window_values(rng):
    """Positive doubles around and inside the window: every exponent within 64 of either boundary and a
    stride through the rest, each with the mantissa patterns, random mantissas and mantissas whose
    leading 20..51 bits are ones (the reciprocal's hard cases next to all ones)."""
    near = set(range(LO - 64, LO + 65)) | set(range(HI - 64, HI + 65))
    exps = sorted(near | set(range(LO, HI, 7)))
    rnd = rng.integers(0, 1 << 52, size=192, dtype=np.uint64)
    ones = np.array([MANT ^ int(rng.integers(0, 1 << (52 - lead))) for lead in range(20, 52)], dtype=np.uint64)
    return _with_exponents(exps, np.concatenate([PATTERNS, rnd, ones]))


def _squares(rng):
    k = np.concatenate([np.arange(1, 2049), rng.integers(1, 1 << 26, size=20000)]).astype(np.float64)
    sq = k * k                                            # exact: k < 2^26
    scaled = sq * 2.0 ** rng.integers(-100, 101, size=sq.size)           # other binades, even and odd shifts
    both = np.concatenate([sq, scaled])
    return np.concatenate([both, np.nextafter(both, 0.0), np.nextafter(both, np.inf)])


def _draw_grid(rng):
    k = np.concatenate([[0, (1 << 52) - 1], rng.integers(0, 1 << 52, size=30000)]).astype(np.uint64)
    u = (k.astype(np.float64) * 2.0 + 1.0) * 2.0 ** -53   # u32pair_unit's expression, every step exact
    return np.concatenate([u, 1.0 - u])


def _outside(rng):
    edge = [_f([np.uint64(e) << np.uint64(52)])[0] for e in (LO, HI)]
    vals = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -2.5e-300, -1e300, 5e-324, 2.2250738585072014e-308,
            np.nextafter(2.2250738585072014e-308, 0.0), 1.7976931348623157e308]
    for b in edge:
        vals += [b, np.nextafter(b, 0.0), np.nextafter(b, np.inf)]
    den = _f(rng.integers(1, 1 << 52, size=4096, dtype=np.uint64))                       # subnormals
    far = _with_exponents(list(range(1, LO - 64, 37)) + list(range(HI + 65, 2047, 37)),
                          np.concatenate([PATTERNS, rng.integers(0, 1 << 52, size=16, dtype=np.uint64)]))
    neg = -_window_values(rng)[::5]
    return np.concatenate([np.array(vals), den, far, neg])


def _inside(x):
    e = (x.view(np.uint64) >> np.uint64(52)).astype(np.int64)      # sign bit included: negatives fall out
    return x[(e >= LO) & (e < HI)]


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(0xF64C0DE)
    win, squares, grid = _window_values(rng), _squares(rng), _draw_grid(rng)
    everything = np.concatenate([win, squares, grid, _outside(rng)])
    assert everything.size <= 1 << 20
    core = np.concatenate([_inside(win), _inside(squares), grid])
    return everything, core


def _check(kind, x, gpu_ctx):
    with np.errstate(all="ignore"):
        want = np.sqrt(x) if kind.startswith("sqrt") else 1.0 / x
    got = gpu.f64_probe(kind, x, ctx=gpu_ctx)
    nan = np.isnan(want)
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~(nan & np.isnan(got)))
    print("%s: %d inputs, %d nan, %d differ" % (kind, x.size, int(nan.sum()), bad.size))
    assert bad.size == 0, [(float.hex(float(x[i])), float.hex(float(got[i])), float.hex(float(want[i]))) for i in bad[:8]]


@pytest.mark.parametrize("kind", ["sqrt_mid", "rcp_mid"])
def test_guarded_helpers_equal_ieee_for_every_input(kind, inputs, gpu_ctx):
    _check(kind, inputs[0], gpu_ctx)


@pytest.mark.parametrize("kind", ["sqrt_core", "rcp_core"])
def test_core_forms_equal_ieee_inside_the_window(kind, inputs, gpu_ctx):
    x = inputs[1]
    assert x.size > 50000 and np.all((x >= 2.0 ** -256) & (x < 2.0 ** 256))
    _check(kind, x, gpu_ctx)
