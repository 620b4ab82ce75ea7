"""The denoiser on the GPU (rt_denoise*, rt_frame.hip) against its NumPy restatement rtamd.denoise.atrous,
on GPU-rendered moments and GPU feature buffers.

The bound: max |device - NumPy| <= 1e-12 * max |out|.  Both sides form the argument of every exp by
correctly rounded operations in the same order, and the two exp implementations are each within 1 ulp; the
output is a ratio of non-negative weighted sums, so weight errors of a few 2^-52 do not amplify; the 1e-10
guard in wl cannot amplify either (a perturbation d of l moves w * du by at most d / e).  Five iterations of
25 taps stay below 1e-13 by this count; 1e-12 leaves a decade."""
import functools

import numpy as np
import pytest
import torch

import adaptive_cases as ac
import feature_cases as fc
from rtamd import denoise, gpu

pytestmark = pytest.mark.gpu

SEED = fc.SEED
PASSES = 16
REL = 1e-12
#: cornell and cover as the issue's frames; 37x23 is no multiple of the 16x16 tile and step 16 reaches past it
FRAMES = [("cornell", 48, 48), ("cover", 64, 36), ("cover", 37, 23)]


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(name, nx, ny):
    """GPU-rendered S, Q, count (16 passes of every pixel) and GPU features (16 passes), read-only host arrays."""
    sc = fc.scene_of(name, nx, ny)
    npx = nx * ny
    S, Q = _dev(np.zeros(npx * 3)), _dev(np.zeros(npx * 3))
    cnt = _dev(np.zeros(npx, dtype=np.uint32))
    pix = _dev(gpu.shard_pixels(nx, ny, 0, 1))
    gpu.render_pixels_device(sc, nx, ny, pix.data_ptr(), npx, 0, PASSES, SEED, S.data_ptr(), Q.data_ptr(), cnt.data_ptr())
    feat = _dev(np.zeros(npx * 8))
    gpu.render_features_device(sc, nx, ny, 0, PASSES, SEED, feat.data_ptr())
    out = (S.cpu().numpy(), Q.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), feat.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


def _device(nx, ny, S, Q, count, n, feat, m, **params):
    d_s, d_f, d_o = _dev(S), _dev(feat), _dev(np.full(nx * ny * 3, -3.0))
    d_q = _dev(Q) if Q is not None else None
    d_c = _dev(count) if count is not None else None
    gpu.denoise_device(nx, ny, gpu.denoise_params(**params), d_s.data_ptr(), d_q.data_ptr() if d_q is not None else None,
                       d_c.data_ptr() if d_c is not None else None, n, d_f.data_ptr(), m, d_o.data_ptr())
    assert np.array_equal(d_s.cpu().numpy(), S, equal_nan=True) and np.array_equal(d_f.cpu().numpy(), feat)   # read only
    return d_o.cpu().numpy()


def _check(label, got, want):
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), label
    scale = np.abs(want[finite]).max()
    err = np.abs(got[finite] - want[finite]).max()
    print("%s: max |device - numpy| = %.3e = %.3e * max |out|" % (label, err, err / scale))
    assert err <= REL * scale, label


@pytest.mark.parametrize("name,nx,ny", FRAMES)
def test_denoise_matches_numpy(sched, name, nx, ny):
    S, Q, cnt, feat = _inputs(name, nx, ny)
    assert (cnt == PASSES).all()
    want = denoise.atrous(S, Q, cnt, 0, feat, PASSES, nx, ny)
    got = _device(nx, ny, S, Q, cnt, 0, feat, PASSES)
    _check("%s %dx%d" % (name, nx, ny), got, want)
    assert np.abs(want - S / PASSES).max() > 1e-3                          # the filter did something
    # count NULL: every pixel has sample_count samples — the same numbers
    assert np.array_equal(_device(nx, ny, S, Q, None, PASSES, feat, PASSES), got)
    # accum2 NULL: no luminance weight, no variance
    _check("%s %dx%d, accum2 NULL" % (name, nx, ny), _device(nx, ny, S, None, None, PASSES, feat, PASSES),
           denoise.atrous(S, None, None, PASSES, feat, PASSES, nx, ny))
    # other parameters than the defaults
    p = dict(iterations=3, normal_squarings=2, sigma_z=0.5, sigma_l=1.5, albedo_floor=0.05)
    _check("%s %dx%d, %r" % (name, nx, ny, p), _device(nx, ny, S, Q, cnt, 0, feat, PASSES, **p),
           denoise.atrous(S, Q, cnt, 0, feat, PASSES, nx, ny, **p))
    # the host entry point gives the device one's bits
    host = gpu.denoise_host(nx, ny, gpu.denoise_params(), S, Q, cnt, 0, feat, PASSES)
    assert np.array_equal(host, got)


def test_denoise_with_an_injected_nan_pixel(sched):
    name, nx, ny = "cover", 37, 23
    S, Q, cnt, feat = (a.copy() for a in _inputs(name, nx, ny))
    j = 11 * nx + 20
    S[3 * j + 1] = np.nan
    want = denoise.atrous(S, Q, cnt, 0, feat, PASSES, nx, ny)
    got = _device(nx, ny, S, Q, cnt, 0, feat, PASSES)
    assert np.isnan(got[3 * j + 1]) and np.isfinite(np.delete(got, 3 * j + 1)).all()
    _check("cover 37x23, NaN pixel", got, want)


def test_denoise_one_pixel_frame(sched):
    S, Q, cnt, feat = _inputs("cornell", 1, 1)
    want = denoise.atrous(S, Q, cnt, 0, feat, PASSES, 1, 1)
    got = _device(1, 1, S, Q, cnt, 0, feat, PASSES)
    _check("cornell 1x1", got, want)


@pytest.mark.parametrize("name,nx,ny", [c for c in ac.CASES if c[0] == "cornell"])
def test_denoise_with_adaptive_counts(sched, name, nx, ny):
    """The moments and the per-pixel counts of an adaptive render (the cases of tests/adaptive_cases.py)."""
    sc = fc.scene_of(name, nx, ny)
    npx = nx * ny
    S, Q = _dev(np.zeros(npx * 3)), _dev(np.zeros(npx * 3))
    cnt = _dev(np.zeros(npx, dtype=np.uint32))
    p = gpu.adaptive_params(ac.TOL, ac.MIN_SPP, ac.MAX_SPP, ac.BATCH_SPP, ac.FLOOR)
    gpu.render_adaptive_device(sc, nx, ny, p, SEED, S.data_ptr(), Q.data_ptr(), cnt.data_ptr())
    S, Q, cnt = S.cpu().numpy(), Q.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)
    assert len(np.unique(cnt)) > 1
    feat = _inputs(name, nx, ny)[3]
    want = denoise.atrous(S, Q, cnt, 0, feat, PASSES, nx, ny)
    _check("%s %dx%d, adaptive counts" % (name, nx, ny), _device(nx, ny, S, Q, cnt, 0, feat, PASSES), want)


def test_scratch_is_sized_again_after_release_pools(sched):
    name, nx, ny = "cornell", 48, 48
    S, Q, cnt, feat = _inputs(name, nx, ny)
    a = _device(nx, ny, S, Q, cnt, 0, feat, PASSES)
    sched.release_pools()
    assert np.array_equal(_device(nx, ny, S, Q, cnt, 0, feat, PASSES), a)


def test_renderer_denoise_end_to_end(sched, tmp_path):
    """Renderer.render + render_features + denoise: the Python layer's buffers reach rt_denoise as they are."""
    from rtamd.render import Renderer
    name, nx, ny = "cornell", 48, 48
    r = Renderer(nx, ny, seed=SEED)
    r.render(fc.scene_of(name, nx, ny), PASSES)
    r.render_features(fc.scene_of(name, nx, ny), PASSES)
    S, _, _, feat = _inputs(name, nx, ny)
    assert np.array_equal(r.raw_data, S) and np.array_equal(r.features, feat)
    out = r.denoise()
    _check("Renderer.denoise", out, denoise.atrous(S, None, None, PASSES, feat, PASSES, nx, ny))
    assert r.albedo.shape == (ny, nx, 3) and r.normal.shape == (ny, nx, 3) and r.depth.shape == (ny, nx)
    assert ((r.hit_fraction >= 0) & (r.hit_fraction <= 1)).all()
    r.save_denoised_as_ppm(str(tmp_path / "d.ppm"))
    assert (tmp_path / "d.ppm").read_text().startswith("P3")
