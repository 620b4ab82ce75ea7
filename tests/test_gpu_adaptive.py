"""Adaptive sampling on the GPU: the selection against NumPy, pixel-list renders against the plain render,
the adaptive driver against a replay of its rounds over one-pass renders (exact) and against the oracle.

The exact comparisons of counts rest on test_adaptive_host.py's oracle replay: with these cases'
parameters no pixel comes within 1e-9 r^2 of the threshold, far more than the device's transcendental
ulps move a colour."""
import functools

import numpy as np
import pytest
import torch

import adaptive_cases as ac
from conftest import host_threads
from rtamd import adaptive, gpu
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4          # as test_gpu_parity
SEED = ac.SEED
SCHEDULES = ["tail", "wavefront"]
POISON_PIX = 0xDEADBEEF
P_ACC, P_ACC2, P_CNT = 0.25, 0.5, 77        # what untouched accum / accum2 / count entries must keep


def _schedule(ctx, schedule):
    if schedule == "wavefront":
        ctx.set_option("tail_off", 1)


def _dev(a):
    """A host array on the device; uint32 travels as int32 bits."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _params(min_spp=ac.MIN_SPP, max_spp=ac.MAX_SPP, batch_spp=ac.BATCH_SPP, tol=ac.TOL, floor=ac.FLOOR):
    return gpu.adaptive_params(tol, min_spp, max_spp, batch_spp, floor)


# ------------------------------------------------------------ 1. selection against NumPy
def _synthetic(npx, seed, max_spp=16):
    """Moments of npx pixels around the threshold of tol 0.1: about half converged, some at max_spp, a few
    zero pixels and NaN moments."""
    rs = np.random.RandomState(seed)
    n = rs.randint(2, max_spp + 1, size=npx).astype(np.uint32)
    mu = rs.uniform(0.01, 1.0, size=(npx, 3))
    sd = mu * rs.uniform(0.0, 0.2, size=(npx, 1)) * np.sqrt(n)[:, None]
    S = mu * n[:, None]
    Q = n[:, None] * (mu * mu + sd * sd)
    z = rs.randint(0, npx, size=max(1, npx // 50))
    S[z] = 0.0
    Q[z] = 0.0
    k = rs.randint(0, npx, size=max(1, npx // 100))
    S[k, rs.randint(0, 3, size=k.size)] = np.nan
    return S, Q, n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1025, 300001])
def test_selection_matches_numpy(gpu_ctx, n):
    tol, floor, max_spp = 0.1, 0.05, 16
    npx = n + 37
    S, Q, cnt = _synthetic(npx, 1000 + n % 997)
    rs = np.random.RandomState(n)
    subset = rs.permutation(npx)[:n].astype(np.uint32)
    finite = np.nan_to_num(S, nan=0.3), Q
    cases = {
        "identity": (None, S, Q, cnt, tol),
        "subset": (subset, S, Q, cnt, tol),
        "all_converged": (subset, finite[0], finite[1], cnt, 1e6),
        "none_converged": (subset, S, Q, np.ones(npx, dtype=np.uint32), tol),
    }
    for label, (lst, Sx, Qx, cx, t) in cases.items():
        d_s, d_q, d_c = _dev(Sx.ravel()), _dev(Qx.ravel()), _dev(cx)
        d_in = _dev(lst) if lst is not None else None
        d_out = _dev(np.full(n, POISON_PIX, dtype=np.uint32))
        m, capped = gpu.adaptive_select_device(d_in.data_ptr() if d_in is not None else None, n, d_s.data_ptr(),
                                               d_q.data_ptr(), d_c.data_ptr(), t, floor, max_spp, d_out.data_ptr())
        pix = lst if lst is not None else np.arange(n, dtype=np.uint32)
        keep = ~adaptive.converged(Sx[pix], Qx[pix], cx[pix], t, floor)
        want = pix[keep]
        got = _u32(d_out)
        print(label, n, "kept", m, "capped", capped)
        assert m == want.size, label
        assert np.array_equal(got[:m], want), label
        assert (got[m:] == POISON_PIX).all(), label
        assert capped == int((cx[want] >= max_spp).sum()), label
        if label == "all_converged":
            assert m == 0
        elif label == "none_converged":
            assert m == n and capped == 0
        elif n > 256:
            assert 0 < m < n and capped > 0
        # the inputs are read only
        assert np.array_equal(d_s.cpu().numpy(), Sx.ravel(), equal_nan=True) and np.array_equal(_u32(d_c), cx)
        if d_in is not None:
            assert np.array_equal(_u32(d_in), lst)


# ------------------------------------------------------------ 2. pixel-list render against the plain render
@functools.lru_cache(maxsize=None)
def _gpu_pass(name, nx, ny, k):
    """Pass k alone from the plain render (0 + x = x), as a read-only (npix, 3) host array."""
    t = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    gpu.render_device(ac.scene_of(name, nx, ny), nx, ny, k, 1, SEED, t.data_ptr())
    a = t.cpu().numpy().reshape(-1, 3)
    a.setflags(write=False)
    return a


def _list_render_case(name, nx, ny, spp_begin, spp_count):
    scene = ac.scene_of(name, nx, ny)
    npx = nx * ny
    lst = np.random.RandomState(npx).permutation(npx)[:npx // 2].astype(np.uint32)
    plain = torch.full((npx * 3,), P_ACC, dtype=torch.float64, device="cuda")
    gpu.render_device(scene, nx, ny, spp_begin, spp_count, SEED, plain.data_ptr())
    acc = torch.full((npx * 3,), P_ACC, dtype=torch.float64, device="cuda")
    acc2 = torch.full((npx * 3,), P_ACC2, dtype=torch.float64, device="cuda")
    cnt = torch.full((npx,), P_CNT, dtype=torch.int32, device="cuda")
    d_lst = _dev(lst)
    h = gpu.render_pixels_device(scene, nx, ny, d_lst.data_ptr(), lst.size, spp_begin, spp_count, SEED, acc.data_ptr(),
                                 acc2.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    listed = np.zeros(npx, dtype=bool)
    listed[lst] = True
    plain, acc, acc2 = (t.cpu().numpy().reshape(-1, 3) for t in (plain, acc, acc2))
    cnt = _u32(cnt)
    assert np.array_equal(acc[listed], plain[listed])
    assert (acc[~listed] == P_ACC).all() and (acc2[~listed] == P_ACC2).all() and (cnt[~listed] == P_CNT).all()
    assert (cnt[listed] == P_CNT + spp_count).all()
    want2 = np.full((npx, 3), P_ACC2)
    for k in range(spp_begin, spp_begin + spp_count):
        x = _gpu_pass(name, nx, ny, k)
        want2 = want2 + x * x
    assert np.array_equal(acc2[listed], want2[listed])
    assert np.array_equal(_u32(d_lst), lst)
    # accum alone (no moments, no counts) takes the same path
    acc_only = torch.full((npx * 3,), P_ACC, dtype=torch.float64, device="cuda")
    gpu.render_pixels_device(scene, nx, ny, d_lst.data_ptr(), lst.size, spp_begin, spp_count, SEED, acc_only.data_ptr())
    assert np.array_equal(acc_only.cpu().numpy().reshape(-1, 3), acc)
    return h, lst.size * spp_count


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name,nx,ny", [("cover", 96, 64), ("cornell", 48, 48), ("curves_small", 64, 36)])
def test_pixel_list_render_bitwise(sched, schedule, name, nx, ny):
    _schedule(sched, schedule)
    _list_render_case(name, nx, ny, 3, 5)


def test_pixel_list_render_through_the_fused_camera_kernel(sched):
    """3072 listed pixels x 16 passes = 49 152 paths in ONE chunk (one lane: two lanes would cut the render
    into two chunks of 24 576, below the 32 768-path tail threshold), so depth 0 runs in the wavefront and
    the fused camera kernel reads the caller's list."""
    sched.set_option("lanes", 1)
    h, paths = _list_render_case("cover", 96, 64, 3, 16)
    st, info = gpu.stats(h), gpu.scene_info(h)
    assert paths > 32768 and st.chunks == 1 and st.paths == paths
    assert info["camera_lds_bytes"] > 0 and st.shade_hits_d0 > 0 and st.finish_paths < paths


def test_zero_length_list_and_zero_passes_do_nothing(sched):
    nx, ny = 8, 8
    scene = ac.scene_of("cornell", nx, ny)
    acc = torch.full((nx * ny * 3,), P_ACC, dtype=torch.float64, device="cuda")
    cnt = torch.full((nx * ny,), P_CNT, dtype=torch.int32, device="cuda")
    d_lst = _dev(np.arange(4, dtype=np.uint32))
    gpu.render_pixels_device(scene, nx, ny, d_lst.data_ptr(), 0, 0, 2, SEED, acc.data_ptr(), None, cnt.data_ptr())
    gpu.render_pixels_device(scene, nx, ny, d_lst.data_ptr(), 4, 0, 0, SEED, acc.data_ptr(), None, cnt.data_ptr())
    torch.cuda.synchronize()
    assert (acc == P_ACC).all() and (cnt == P_CNT).all()


# ------------------------------------------------------------ 3. an entry outside the frame
def test_list_entry_outside_the_frame_is_refused(sched):
    """Only the read-only range check runs: no kernel that writes through the list is launched."""
    nx, ny = 16, 12
    scene = ac.scene_of("cornell", nx, ny)
    lst = np.arange(40, dtype=np.uint32)
    lst[17] = nx * ny
    acc = torch.full((nx * ny * 3,), P_ACC, dtype=torch.float64, device="cuda")
    acc2 = torch.full((nx * ny * 3,), P_ACC2, dtype=torch.float64, device="cuda")
    cnt = torch.full((nx * ny,), P_CNT, dtype=torch.int32, device="cuda")
    d_lst = _dev(lst)
    with pytest.raises(RtError, match="entry %d " % (nx * ny)):
        gpu.render_pixels_device(scene, nx, ny, d_lst.data_ptr(), lst.size, 0, 2, SEED, acc.data_ptr(), acc2.data_ptr(),
                                 cnt.data_ptr())
    torch.cuda.synchronize()
    assert (acc == P_ACC).all() and (acc2 == P_ACC2).all() and (cnt == P_CNT).all()
    assert np.array_equal(_u32(d_lst), lst)


# ------------------------------------------------------------ 4. the driver against a replay of its rounds
def _adaptive_gpu(name, nx, ny, params):
    """rt_render_adaptive_device into buffers holding garbage (the call overwrites all three)."""
    npx = nx * ny
    acc = torch.full((npx * 3,), 7.5, dtype=torch.float64, device="cuda")
    acc2 = torch.full((npx * 3,), -3.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((npx,), 99, dtype=torch.int32, device="cuda")
    res = gpu.render_adaptive_device(ac.scene_of(name, nx, ny), nx, ny, params, SEED, acc.data_ptr(), acc2.data_ptr(),
                                     cnt.data_ptr())
    torch.cuda.synchronize()
    return acc.cpu().numpy().reshape(-1, 3), acc2.cpu().numpy().reshape(-1, 3), _u32(cnt), res


@functools.lru_cache(maxsize=None)
def _self_replay(name, nx, ny):
    passes = [_gpu_pass(name, nx, ny, k) for k in range(ac.MAX_SPP)]
    return adaptive.replay(passes, ac.MIN_SPP, ac.MAX_SPP, ac.BATCH_SPP, ac.TOL, ac.FLOOR)


def _assert_is_replay(name, nx, ny, got):
    acc, acc2, cnt, res = got
    S, Q, count, rounds, capped = _self_replay(name, nx, ny)
    assert np.array_equal(cnt, count)
    assert np.array_equal(acc, S) and np.array_equal(acc2, Q)
    assert res["rounds"] == rounds and res["samples"] == int(count.sum(dtype=np.uint64))
    assert res["pixels_capped"] == capped and res["pixels_converged"] == nx * ny - capped
    assert res["ms_total"] >= res["ms_select"] >= 0.0


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name,nx,ny", ac.CASES)
def test_adaptive_matches_self_replay(sched, schedule, name, nx, ny):
    _schedule(sched, schedule)
    got = _adaptive_gpu(name, nx, ny, _params())
    hist = [int((got[2] == c).sum()) for c in range(ac.MIN_SPP, ac.MAX_SPP + 1, ac.BATCH_SPP)]
    print(name, hist, got[3])
    assert all(h > 0 for h in hist)
    _assert_is_replay(name, nx, ny, got)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name,nx,ny", ac.CASES)
def test_adaptive_with_min_equal_max_is_the_plain_render(sched, schedule, name, nx, ny):
    _schedule(sched, schedule)
    acc, acc2, cnt, res = _adaptive_gpu(name, nx, ny, _params(min_spp=6, max_spp=6))
    plain = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    gpu.render_device(ac.scene_of(name, nx, ny), nx, ny, 0, 6, SEED, plain.data_ptr())
    assert np.array_equal(acc, plain.cpu().numpy().reshape(-1, 3))
    assert (cnt == 6).all() and res["rounds"] == 1 and res["samples"] == 6 * nx * ny
    assert res["pixels_converged"] + res["pixels_capped"] == nx * ny


# ------------------------------------------------------------ 5. the driver against the oracle
@pytest.mark.parametrize("name,nx,ny", ac.CASES)
def test_adaptive_matches_oracle(sched, oracle_mod, name, nx, ny):
    acc, _, cnt, _ = _adaptive_gpu(name, nx, ny, _params())
    npx = nx * ny
    allow = max(2, npx // 200)
    o = ac.oracle_scene(name, nx, ny)
    ref = np.zeros(npx * 3)
    for n in np.unique(cnt):
        o.render_pixels(nx, ny, 0, int(n), SEED, ref, np.nonzero(cnt == n)[0].astype(np.uint32), nthreads=host_threads())
    a = acc / cnt[:, None]
    b = ref.reshape(-1, 3) / cnt[:, None]
    rms = float(np.sqrt(np.mean((a - b) ** 2)))
    nbad = int((np.abs(a - b).max(axis=1) > 1e-9).sum())
    _, _, count_orc, _, _ = adaptive.replay(ac.oracle_passes(name, nx, ny), ac.MIN_SPP, ac.MAX_SPP, ac.BATCH_SPP, ac.TOL,
                                            ac.FLOOR)
    ndiff = int((cnt != count_orc).sum())
    print("%s: rms=%.3e pixels>1e-9: %d/%d counts differing: %d" % (name, rms, nbad, npx, ndiff))
    assert np.isfinite(acc).all() and rms <= RMS_TOL
    assert nbad <= allow
    assert ndiff <= allow


# ------------------------------------------------------------ 6. schedule invariance
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("option,value", [("max_paths", 1024), ("lanes", 1), ("lanes", 2)])
@pytest.mark.parametrize("name,nx,ny", ac.CASES)
def test_adaptive_is_schedule_invariant(sched, schedule, option, value, name, nx, ny):
    _schedule(sched, schedule)
    sched.set_option(option, value)
    _assert_is_replay(name, nx, ny, _adaptive_gpu(name, nx, ny, _params()))


# ------------------------------------------------------------ 7. the device resolve with counts
@pytest.mark.parametrize("name,nx,ny", ac.CASES)
def test_device_resolve_with_counts_matches_host(sched, name, nx, ny):
    S, _, count, _, _ = _self_replay(name, nx, ny)
    count = count.copy()
    count[::97] = 0                                  # never-sampled pixels resolve to 0
    d_s, d_c = _dev(S.ravel()), _dev(count)
    out = torch.full((nx * ny * 3,), 201, dtype=torch.uint8, device="cuda")
    gpu.resolve_u8_counts_device(d_s.data_ptr(), d_c.data_ptr(), nx, ny, out.data_ptr())
    got = out.cpu().numpy()
    assert np.array_equal(got, gpu.resolve_u8_counts(S, count, nx, ny))
    assert not got.reshape(-1, 3)[count == 0].any() and got.any()


# ------------------------------------------------------------ 8. the Python Renderer
def test_renderer_render_adaptive(sched):
    from rtamd.render import Renderer
    name, nx, ny = ac.CASES[0]
    r = Renderer(nx, ny, seed=SEED)
    res = r.render_adaptive(ac.scene_of(name, nx, ny), ac.TOL, min_spp=ac.MIN_SPP, max_spp=ac.MAX_SPP,
                            batch_spp=ac.BATCH_SPP, floor=ac.FLOOR)
    acc, acc2, cnt, res_dev = _adaptive_gpu(name, nx, ny, _params())
    assert np.array_equal(r.raw_data.reshape(-1, 3), acc) and np.array_equal(r.raw_data2.reshape(-1, 3), acc2)
    assert np.array_equal(r.counts, cnt) and r.sample_count == int(cnt.max()) == ac.MAX_SPP
    assert np.array_equal(r.image, gpu.resolve_u8_counts(acc, cnt, nx, ny))
    for k in ("rounds", "samples", "pixels_converged", "pixels_capped"):
        assert res[k] == res_dev[k]
