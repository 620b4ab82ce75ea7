"""The denoiser's rule in NumPy (include/rt.h, "denoiser").

The same f64 operations in the same order as the device's kernels
(rt_frame.hip k_denoise_prepare / k_denoise_atrous): the library is built
without FMA contraction and f64 division and sqrt are correctly rounded, so
``atrous`` differs from ``rt_denoise`` only by the two exp implementations
(each within 1 ulp).

S, Q: (ny, nx, 3) or flat running sums of the samples and of their squares (Q
may be None); count: per-pixel sample counts or None (every pixel has
``sample_count``); feat: the (ny*nx, 8) feature sums of ``feat_count`` passes.
"""
import numpy as np

#: the defaults of Renderer.denoise (the prototype's; tools/denoise_report.py records what was tried)
DEFAULTS = dict(iterations=5, normal_squarings=7, sigma_z=0.1, sigma_l=4.0, albedo_floor=1e-2)
#: the B3-spline kernel at offsets -2 .. 2
KERNEL = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def check_params(iterations, normal_squarings, sigma_z, sigma_l, albedo_floor):
    """rt_denoise's refusals."""
    if not 1 <= int(iterations) <= 12:
        raise ValueError("iterations must be in 1 .. 12")
    if not 0 <= int(normal_squarings) <= 16:
        raise ValueError("normal_squarings must be in 0 .. 16")
    for name, v in (("sigma_z", sigma_z), ("sigma_l", sigma_l), ("albedo_floor", albedo_floor)):
        if not np.isfinite(v) or not v > 0.0:
            raise ValueError("%s must be finite and > 0" % name)


def prepare(S, Q, count, sample_count, feat, feat_count, nx, ny, albedo_floor):
    """Per pixel (ny, nx, ...): the demodulated signal u, the variance v of its mean, the divisor den and
    the guides N, z, h."""
    S = np.asarray(S, dtype=np.float64).reshape(ny, nx, 3)
    f = np.asarray(feat, dtype=np.float64).reshape(ny, nx, 8)
    if feat_count < 1:
        raise ValueError("feat_count must be >= 1")
    m = np.float64(feat_count)
    if count is None:
        n = np.full((ny, nx), np.float64(sample_count))
    else:
        n = np.asarray(count).reshape(ny, nx).astype(np.float64)
    with np.errstate(all="ignore"):
        a = f[..., 0:3] / m
        N = f[..., 3:6] / m
        z = f[..., 6] / m
        h = f[..., 7] / m
        den = np.where(a > albedo_floor, a, np.float64(albedo_floor))
        c = np.where((n == 0.0)[..., None], 0.0, S / n[..., None])
        u = c / den
        v = np.zeros((ny, nx))
        if Q is not None:
            Q = np.asarray(Q, dtype=np.float64).reshape(ny, nx, 3)
            nn = n * (n - 1.0)
            e = []
            for k in range(3):
                d = Q[..., k] - (S[..., k] * S[..., k]) / n
                e.append((np.where(d < 0.0, 0.0, d) / nn) / (den[..., k] * den[..., k]))
            v = np.where(n >= 2.0, (e[0] + e[1]) + e[2], 0.0)
    return u, v, den, N, z, h


def _shift(a, oy, ox, ys, xs):
    """a[y + oy, x + ox] for the destination window (ys, xs)."""
    return a[ys.start + oy:ys.stop + oy, xs.start + ox:xs.stop + ox]


def iterate(u, v, N, z, h, step, normal_squarings, sigma_z, sigma_l, use_l):
    """One a-trous iteration at ``step``: returns (u', v')."""
    ny, nx = v.shape
    valid = np.isfinite(u).all(axis=-1) & np.isfinite(v)
    l = (u[..., 0] + u[..., 1]) + u[..., 2]
    W = np.zeros((ny, nx))
    U = np.zeros((ny, nx, 3))
    V = np.zeros((ny, nx))
    with np.errstate(all="ignore"):
        lden = np.float64(sigma_l) * np.sqrt(v) + 1e-10
        for dy in range(-2, 3):
            oy = dy * step
            if abs(oy) >= ny:
                continue
            ys = slice(max(0, -oy), min(ny, ny - oy))          # destination rows whose tap is inside
            for dx in range(-2, 3):
                ox = dx * step
                if abs(ox) >= nx:
                    continue
                xs = slice(max(0, -ox), min(nx, nx - ox))
                hk = np.float64(KERNEL[dy + 2]) * np.float64(KERNEL[dx + 2])
                uq = _shift(u, oy, ox, ys, xs)
                vq = _shift(v, oy, ox, ys, xs)
                if dx == 0 and dy == 0:
                    w = np.full(vq.shape, hk)
                    use = np.ones(vq.shape, dtype=bool)
                else:
                    use = _shift(valid, oy, ox, ys, xs)
                    Np, Nq = N[ys, xs], _shift(N, oy, ox, ys, xs)
                    g = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                    wn = np.where(g > 0.0, g, 0.0)
                    for _ in range(int(normal_squarings)):
                        wn = wn * wn
                    wn = np.where((h[ys, xs] == 0.0) & (_shift(h, oy, ox, ys, xs) == 0.0), 1.0, wn)
                    zp, zq = z[ys, xs], _shift(z, oy, ox, ys, xs)
                    zm = np.where(zp > zq, zp, zq)
                    wz = np.exp(-(np.abs(zp - zq) / (np.float64(sigma_z) * zm + 1e-300)))
                    if use_l:
                        wl = np.exp(-(np.abs(l[ys, xs] - _shift(l, oy, ox, ys, xs)) / lden[ys, xs]))
                    else:
                        wl = 1.0
                    w = ((hk * wn) * wz) * wl
                W[ys, xs] = np.where(use, W[ys, xs] + w, W[ys, xs])
                U[ys, xs] = np.where(use[..., None], U[ys, xs] + w[..., None] * uq, U[ys, xs])
                V[ys, xs] = np.where(use, V[ys, xs] + (w * w) * vq, V[ys, xs])
        un = U / W[..., None]
        vn = V / (W * W)
    un = np.where(valid[..., None], un, u)                       # a pixel that is not valid passes through
    vn = np.where(valid, vn, v)
    return un, vn


def atrous(S, Q, count, sample_count, feat, feat_count, nx, ny, iterations=DEFAULTS["iterations"],
           normal_squarings=DEFAULTS["normal_squarings"], sigma_z=DEFAULTS["sigma_z"], sigma_l=DEFAULTS["sigma_l"],
           albedo_floor=DEFAULTS["albedo_floor"]):
    """rt_denoise on the host: the filtered per-pixel mean radiance, (ny*nx*3,) float64."""
    check_params(iterations, normal_squarings, sigma_z, sigma_l, albedo_floor)
    u, v, den, N, z, h = prepare(S, Q, count, sample_count, feat, feat_count, nx, ny, albedo_floor)
    for i in range(int(iterations)):
        u, v = iterate(u, v, N, z, h, 1 << i, normal_squarings, sigma_z, sigma_l, Q is not None)
    with np.errstate(all="ignore"):
        return (u * den).reshape(-1)
