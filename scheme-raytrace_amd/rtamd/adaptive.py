"""The adaptive render's stop rule in NumPy (include/rt.h, "adaptive sampling").

The same f64 operations in the same order as the device's: the library is
built without FMA contraction and f64 division is correctly rounded, so
``converged`` reproduces the selection kernels' verdicts bit for bit.

S, Q: (..., 3) running sums of the samples and of their squares; n: (...)
sample counts.
"""
import numpy as np


def _terms(S, Q, n, floor):
    S = np.asarray(S, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = np.asarray(n).astype(np.float64)
    with np.errstate(all="ignore"):
        nn = n * (n - 1.0)
        v = []
        for c in range(3):
            d = Q[..., c] - (S[..., c] * S[..., c]) / n
            v.append(np.where(d < 0.0, 0.0, d) / nn)       # (d < 0 ? 0 : d): a NaN moment stays a NaN
        e2 = (v[0] + v[1]) + v[2]
        m = ((S[..., 0] + S[..., 1]) + S[..., 2]) / n
        b = np.where(m > floor, m, np.float64(floor))
    return e2, b


def converged(S, Q, n, tol, floor):
    """e2 <= (tol*b)^2: the squared standard error of the pixel mean (channels summed) against the
    relative tolerance on b = max(mean of the channel sum, floor).  A NaN compares false."""
    e2, b = _terms(S, Q, n, floor)
    with np.errstate(all="ignore"):
        r = np.float64(tol) * b
        return e2 <= r * r


def relative_error(S, Q, n, floor):
    """sqrt(e2) / b: the quantity ``tol`` bounds."""
    e2, b = _terms(S, Q, n, floor)
    with np.errstate(all="ignore"):
        return np.sqrt(e2) / b


def replay(samples, min_spp, max_spp, batch_spp, tol, floor):
    """The adaptive rounds over per-pass colours samples[k] (k < max_spp; each (npix, 3)): returns
    (S, Q, count, rounds, capped) as rt_render_adaptive computes them — sums in pass order, a pixel leaves
    after the first round that finds it converged."""
    npix = samples[0].shape[0]
    S = np.zeros((npix, 3))
    Q = np.zeros((npix, 3))
    count = np.zeros(npix, dtype=np.uint32)
    active = np.ones(npix, dtype=bool)
    done = rounds = 0
    while active.any() and done < max_spp:
        passes = min_spp if done == 0 else min(batch_spp, max_spp - done)
        for k in range(done, done + passes):
            x = np.asarray(samples[k], dtype=np.float64)[active]
            S[active] = S[active] + x
            Q[active] = Q[active] + x * x
        count[active] += np.uint32(passes)
        done += passes
        rounds += 1
        active &= ~converged(S, Q, count, tol, floor)
    return S, Q, count, rounds, int(active.sum())
