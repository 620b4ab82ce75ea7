"""First-hit feature buffers on the GPU (rt_render_features*, k_features): bit for bit against the oracle
features helper (tests/feature_cases.py), and the invariances a running sum over (seed, pixel, pass)
keyed camera samples must have."""
import functools

import numpy as np
import pytest
import torch

import feature_cases as fc
from rtamd import gpu
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

SEED = fc.SEED
SENTINEL = -7.25
#: scenes of the invariance tests; cornell_smoke (constant media, whose hit test draws from the ray's
#: stream) is checked only here: the oracle's hit probe cannot draw for a medium
INVARIANCE_CASES = [("cornell", 48, 48), ("cover_marble", 32, 18), ("curves_small", 48, 32), ("cornell_smoke", 32, 32)]


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _features(name, nx, ny, spp_begin, spp_count, start=None, pix=None, ctx=None):
    """The (nx*ny, 8) device result of one call, starting from zeros or from `start`."""
    feat = _dev(np.zeros(nx * ny * 8) if start is None else start.ravel())
    d_pix = _dev(pix) if pix is not None else None
    gpu.render_features_device(fc.scene_of(name, nx, ny), nx, ny, spp_begin, spp_count, SEED, feat.data_ptr(),
                               d_pix.data_ptr() if d_pix is not None else None, 0 if pix is None else pix.size, ctx=ctx)
    return feat.cpu().numpy().reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def _whole(name, nx, ny, passes):
    f = _features(name, nx, ny, 0, passes)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("name,nx,ny", fc.FEATURE_CASES)
def test_features_match_the_oracle_bit_for_bit(sched, oracle_mod, name, nx, ny):
    """Passes 0..3: a pixel passes when all eight sums are bit-equal; at most passes*npix/1000 pixels may
    differ (the per-ray allowance test_hit_rays_vs_oracle_hit_world grants for equal-t ties; each such ray
    can spoil one pixel).  No tolerance on any channel."""
    passes = fc.FEATURE_PASSES
    want = fc.oracle_features(name, nx, ny, passes)
    got = _whole(name, nx, ny, passes)
    bad = np.flatnonzero((got != want).any(axis=1))
    allowed = passes * nx * ny // 1000
    print("%s %dx%d: %d of %d pixels differ (allowed %d)" % (name, nx, ny, bad.size, nx * ny, allowed))
    for j in bad[:12]:
        print("  pixel %d (x %d, y %d): gpu %r\n%soracle %r" % (j, j % nx, j // nx, got[j].tolist(), " " * 24, want[j].tolist()))
    assert np.isfinite(got).all()
    assert bad.size <= allowed


@pytest.mark.parametrize("name,nx,ny", INVARIANCE_CASES)
def test_feature_sums_do_not_depend_on_batching_or_lists(sched, name, nx, ny):
    npx = nx * ny
    one = _whole(name, nx, ny, 8)
    assert ((one[:, 7] >= 0) & (one[:, 7] <= 8)).all()                     # hits <= passes
    # 8 passes in one call == 8 calls of one pass == 3 + 5
    f = np.zeros((npx, 8))
    for k in range(8):
        f = _features(name, nx, ny, k, 1, start=f)
    assert np.array_equal(f, one)
    assert np.array_equal(_features(name, nx, ny, 3, 5, start=_features(name, nx, ny, 0, 3)), one)
    # about 300 unique, shuffled pixels: exactly the whole-frame values, every other record at the sentinel
    rs = np.random.RandomState(nx * 1000 + ny)
    pix = rs.permutation(npx)[:min(300, npx - 5)].astype(np.uint32)
    listed = np.zeros(npx, dtype=bool)
    listed[pix] = True
    start = np.full((npx, 8), SENTINEL)
    start[listed] = 0.0
    got = _features(name, nx, ny, 0, 8, start=start, pix=pix)
    assert np.array_equal(got[listed], one[listed])
    assert (got[~listed] == SENTINEL).all()
    # the host variant equals the device variant
    host = np.zeros(npx * 8)
    gpu.render_features_host(fc.scene_of(name, nx, ny), nx, ny, 0, 8, SEED, host)
    assert np.array_equal(host.reshape(-1, 8), one)
    # nothing to do: an empty list, no passes
    d, d_pix = _dev(np.full(npx * 8, SENTINEL)), _dev(pix)
    gpu.render_features_device(fc.scene_of(name, nx, ny), nx, ny, 0, 0, SEED, d.data_ptr())
    gpu.render_features_device(fc.scene_of(name, nx, ny), nx, ny, 0, 4, SEED, d.data_ptr(), d_pix.data_ptr(), 0)
    assert (d.cpu().numpy() == SENTINEL).all()


def test_a_list_entry_outside_the_frame_fails_and_leaves_feat_untouched(sched):
    name, nx, ny = "cornell", 48, 48
    pix = np.arange(64, dtype=np.uint32)
    pix[17] = nx * ny
    d, d_pix = _dev(np.full(nx * ny * 8, SENTINEL)), _dev(pix)
    with pytest.raises(RtError, match="outside the frame"):
        gpu.render_features_device(fc.scene_of(name, nx, ny), nx, ny, 0, 2, SEED, d.data_ptr(), d_pix.data_ptr(), pix.size)
    assert (d.cpu().numpy() == SENTINEL).all()


def test_a_features_call_leaves_renders_as_they_were(sched):
    """rt_render_device of the same passes before and after a features call on the same scene is
    bit-identical: the pools, the cached pixel list and the fault word are undisturbed."""
    name, nx, ny = "cover", 64, 36
    sc = fc.scene_of(name, nx, ny)

    def render():
        acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda:0")
        gpu.render_device(sc, nx, ny, 0, 4, SEED, acc.data_ptr())
        return acc.cpu().numpy()

    before = render()
    _features(name, nx, ny, 0, 4)
    pix = np.arange(100, dtype=np.uint32)
    _features(name, nx, ny, 2, 3, pix=pix)
    assert np.array_equal(render(), before)
