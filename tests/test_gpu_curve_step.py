"""One step of the persistent curve extend, record by record, against the oracle (tests/curve_step_cases.py).

rt_step_rays on a curve-kernel scene runs the iteration a render runs: launch_extend picks k_extend_curves<0> (per-wave
ray claiming, candidate batches, the LDS stack column and its overflow area, spilling appends into the hit queues),
then launch_shade per material.  The oracle's orc_step performs the same segment.  With the exact libm (these scenes'
default) every field is the same double: the queued hit's t, hit or miss, the survivor's origin, direction,
throughput and counter, the written colour; every record ends exactly one way and the survivor counters add up.
The material is exact on `dup` and `flat` (there the tie rule is the subject) and elsewhere within the n // 1000
allowance of test_gpu_hit_walks._check, at an equal t.

The comparison is test_gpu_scatter.step_and_check's, field for field (scatter_cases.expect / same_bits), with that
allowance added and the differing fields counted for the report (tools/curve_step_report.py).

Further: the launch shapes at which this kernel can differ (prefixes around a wave and a block, 2049 records, one and
three blocks, depth 0 / 1 / 2 / 99 / 100, counters 0..7, the LDS stack column cut to one entry); the persistent kernel
against the per-lane k_extend<kFeatCurves> and the flat list, bit for bit in both libm modes; RT_STEP_FUSED
(k_extend_curves<FUSE>, both instances) against the iterated step, with its ring under pressure; RT_STEP_TAIL on
curve scenes; the group-path curve and the Klein set; and the refusals.
"""
import numpy as np
import pytest

import curve_step_cases as cc
import scatter_cases as sc
from rtamd import gpu
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

FIELDS = ("ends exactly one way", "hit t", "hit or miss", "hit material", "survives", "survivor origin",
          "survivor direction", "survivor throughput", "survivor counter", "colour")
EXACT_MAT = ("dup", "flat")
_expect = {}


def expect(oracle_mod, name, rays, ctr, depth, T):
    key = (name, rays.tobytes(), ctr.tobytes(), depth, T.tobytes())
    if key not in _expect:
        _expect[key] = sc.expect(cc.oracle_scene(oracle_mod, name), rays, depth, T=T, ctr=ctr)
    return _expect[key]


def compare(r, e, n, exact_mat):
    """{field: records that differ} between a StepResult and the oracle's Expect (test_gpu_scatter.step_and_check's
    fields).  The material may differ on n // 1000 records whose t is the oracle's (a tie), unless exact_mat."""
    entries, wrote = r.entries(), r.wrote()
    bad = {}
    bad["ends exactly one way"] = (entries + wrote.astype(np.int32)) != 1
    bad["hit t"] = ~sc.same_bits(r.t, e.t)
    bad["hit or miss"] = (r.mat < 0) != (e.mat < 0)
    mat = r.mat != e.mat
    if not exact_mat and mat.sum() <= n // 1000 and not (mat & (bad["hit t"] | bad["hit or miss"])).any():
        mat = np.zeros(n, dtype=bool)
    bad["hit material"] = mat
    bad["survives"] = (entries == 1) != e.survive
    s = e.survive & (entries == 1)
    bad["survivor origin"] = ~sc.same_bits(r.ray[:, 0:3], e.ray[:, 0:3]).all(axis=1) & s
    bad["survivor direction"] = ~sc.same_bits(r.ray[:, 3:6], e.ray[:, 3:6]).all(axis=1) & s
    bad["survivor throughput"] = ~sc.same_bits(r.T, e.T).all(axis=1) & s
    bad["survivor counter"] = (r.ctr != e.ctr) & s
    bad["colour"] = ~sc.same_bits(r.color, e.color).all(axis=1) & ~e.survive & wrote
    return bad


def step(scene, rays, ctr, depth, T, **kw):
    return gpu.step_rays(scene, rays, T_in=T, ctr_in=ctr, seed=sc.SEED, smp=sc.SMP, depth=depth, **kw)


def step_and_check(oracle_mod, name, rays, ctr, depth, cls="", scene=None, want_extend=gpu.EXTEND_CURVES, tag=""):
    """One step of the records against the oracle; returns (StepResult, Expect, the number of differing fields)."""
    n = len(rays)
    T = sc.throughputs(n, depth)
    e = expect(oracle_mod, name, rays, ctr, depth, T)
    r = step(scene or cc.scene(name), rays, ctr, depth, T)
    bad = compare(r, e, n, cls in EXACT_MAT)
    curve = int(cc.curve_hits(name, e.rows, rays).sum())
    ndiff = sum(int(b.sum()) for b in bad.values())
    print("%-15s %-9s %-12s depth %3d n %5d curve hits %4d survive %4d wrote %4d extend %d: %s" % (
        name, cls, tag, depth, n, curve, int(e.survive.sum()), int(r.wrote().sum()), r.extend,
        ", ".join("%s %d" % (k, int(b.sum())) for k, b in bad.items() if b.any()) or "all equal"))
    assert r.extend == want_extend, (name, r.extend)
    for what, b in bad.items():
        k = np.flatnonzero(b)[:3]
        assert not b.any(), (name, cls, tag, what, int(b.sum()),
                             [(int(i), rays[i].tolist(), int(ctr[i]), float(e.t[i]), float(r.t[i]), int(e.mat[i]), int(r.mat[i]))
                              for i in k])
    assert r.survivors == int(e.survive.sum()) == int(r.entries().sum()), (name, cls, r.survivors, int(e.survive.sum()))
    return r, e, ndiff


def same_result(a, b):
    """Two StepResults, bit for bit in every output."""
    out = {}
    for f in ("status", "ctr", "mat"):
        out[f] = getattr(a, f) != getattr(b, f)
    for f in ("color", "ray", "T"):
        out[f] = ~sc.same_bits(getattr(a, f), getattr(b, f)).all(axis=1)
    out["t"] = ~sc.same_bits(a.t, b.t)
    out["survivors"] = np.array([a.survivors != b.survivors])
    return {k: int(v.sum()) for k, v in out.items() if v.any()}


def iterate_steps(scene, rays, ctr, depth, T):
    """RT_STEP_STEP iterated to the end of every path (test_gpu_scatter.iterate_steps with the records' counters):
    (colours (n, 3), the continuation segments: the survivors of every round)."""
    n = len(rays)
    out = np.full((n, 3), np.nan)
    done = np.zeros(n, dtype=bool)
    cur, ctr, pix = rays.copy(), ctr.copy(), np.arange(n, dtype=np.uint32)
    segs = 0
    for rnd in range(sc.KMAX + 2):
        if len(cur) == 0:
            break
        r = gpu.step_rays(scene, cur, T_in=T, ctr_in=ctr, pix=pix, seed=sc.SEED, smp=sc.SMP, depth=depth + rnd)
        assert ((r.entries() + r.wrote()) == 1).all()
        w = r.wrote()
        assert not done[pix[w]].any()
        out[pix[w]] = r.color[w]
        done[pix[w]] = True
        s = ~w
        segs += int(s.sum())
        cur = np.concatenate([r.ray[s], np.zeros((int(s.sum()), 1))], axis=1)
        T, ctr, pix = r.T[s], r.ctr[s], pix[s]
    assert len(cur) == 0 and done.all()
    return out, segs


_iterated = {}


def iterated(name, key, rays, ctr, depth, T):
    """iterate_steps once per (scene, records, libm) and module."""
    if (name, key) not in _iterated:
        _iterated[(name, key)] = iterate_steps(cc.scene(name), rays, ctr, depth, T)
    return _iterated[(name, key)]


# ------------------------------------------------------------------ one step against the oracle
@pytest.mark.parametrize("name", list(cc.CASES))
def test_one_step_vs_oracle(sched, oracle_mod, name):
    """Every class of a curve-kernel scene through k_extend_curves<0> and the shades (depth 1; `moving` at depth 0)."""
    total = 0
    for cls, r in cc.records(oracle_mod, name).items():
        total += step_and_check(oracle_mod, name, r.rays, r.ctr, 0 if cls == "moving" else 1, cls)[2]
    assert total == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_launch_shapes(sched, oracle_mod, monkeypatch, n):
    """Prefixes of the mixed records around a wave, a block and (2049) nine blocks; the grid as launch_extend sizes
    it, one block (every record claimed by four waves, their appends spilling between shards) and three: the
    oracle's fields each time, and the same outputs bit for bit."""
    rays, ctr = cc.mixed(oracle_mod, "curve_mix", n)
    runs = []
    for blocks in (None, "1", "3"):
        monkeypatch.delenv("RTAMD_CURVE_BLOCKS", raising=False)
        if blocks:
            monkeypatch.setenv("RTAMD_CURVE_BLOCKS", blocks)
        runs.append(step_and_check(oracle_mod, "curve_mix", rays, ctr, 1, "mixed", tag="blocks %s" % blocks)[0])
    assert runs[0].status.shape == (n,)
    for other in runs[1:]:
        assert same_result(runs[0], other) == {}


@pytest.mark.parametrize("depth", [0, 1, 2, sc.KMAX - 1, sc.KMAX])
def test_depths(sched, oracle_mod, depth):
    """Depth 0: the contiguous raygen state, ray times read (`moving` joins the records); depth 1 and 2: the sharded
    survivor view in either state pool; kMaxDepth - 1 and kMaxDepth, where only lights and the sky write colour."""
    for name in ("curve_mix", "curves_small"):
        rays, ctr = cc.mixed(oracle_mod, name)
        if depth == 0 and name == "curve_mix":
            m = cc.records(oracle_mod, name)["moving"]
            rays, ctr = np.concatenate([rays, m.rays]), np.concatenate([ctr, m.ctr])
        r = step_and_check(oracle_mod, name, rays, ctr, depth, "mixed")[0]
        if depth == sc.KMAX:
            assert r.survivors == 0 and r.wrote().all()


@pytest.mark.parametrize("ctr0", range(8))
def test_counter_phases(sched, oracle_mod, ctr0):
    rays, ctr = cc.mixed(oracle_mod, "curve_mix")
    ctr = ctr + ((np.arange(len(rays), dtype=np.uint32) % 3) * 8 + ctr0).astype(np.uint32)
    step_and_check(oracle_mod, "curve_mix", rays, ctr, 1, "mixed", tag="ctr %d" % ctr0)


def test_lds_stack_column_cut_to_one_entry(sched, oracle_mod, monkeypatch):
    """RTAMD_CURVE_LDS_STACK=1 (read at the commit, as test_curve_walk_stack_overflow_bitwise sets it): every push past
    the first goes to the overflow area, and the step's outputs do not change by a bit."""
    from rtamd import scenes
    rays, ctr = cc.mixed(oracle_mod, "curves_small")
    base = step_and_check(oracle_mod, "curves_small", rays, ctr, 1, "mixed")[0]
    monkeypatch.setenv("RTAMD_CURVE_LDS_STACK", "1")
    cut = scenes.cornell_curves_small(cc.NX, cc.NY)
    info = gpu.scene_info(gpu.upload(cut))
    assert info["curve_stack"] > 1, info
    for blocks in (None, "1"):
        if blocks:
            monkeypatch.setenv("RTAMD_CURVE_BLOCKS", blocks)
        low = step_and_check(oracle_mod, "curves_small", rays, ctr, 1, "mixed", scene=cut, tag="lds stack 1")[0]
        assert same_result(base, low) == {}


# ------------------------------------------------------------------ persistent against per-lane
_flat_list = {}


def _flat_list_scene(name, monkeypatch):
    """The scene committed as the flat list (RTAMD_BVH_MIN above every count, read at the commit): once per module."""
    if name not in _flat_list:
        monkeypatch.setenv("RTAMD_BVH_MIN", "1000000000")
        s = cc.CASES[name][0](cc.NX, cc.NY)
        gpu.upload(s)
        monkeypatch.delenv("RTAMD_BVH_MIN")
        _flat_list[name] = s
    return _flat_list[name]


@pytest.mark.parametrize("libm", ["exact", "device"])
@pytest.mark.parametrize("name", ["curve_mix", "dup"])
def test_persistent_vs_per_lane(sched, oracle_mod, monkeypatch, name, libm):
    """k_extend_curves<0>, the per-lane k_extend<kFeatCurves> over the same tree (RTAMD_CURVE_BLOCKS=0) and the flat
    list give the same outputs bit for bit, in both libm modes (under the device libm this is the only requirement:
    the oracle's sin / cos are the exact ones)."""
    sched.set_option("exact_libm", libm)
    rays, ctr = cc.mixed(oracle_mod, name)
    T = sc.throughputs(len(rays), 1)
    a = step(cc.scene(name), rays, ctr, 1, T)
    assert a.extend == gpu.EXTEND_CURVES
    monkeypatch.setenv("RTAMD_CURVE_BLOCKS", "0")
    b = step(cc.scene(name), rays, ctr, 1, T)
    monkeypatch.delenv("RTAMD_CURVE_BLOCKS")
    c = step(_flat_list_scene(name, monkeypatch), rays, ctr, 1, T)
    assert b.extend == gpu.EXTEND_PER_RAY and c.extend == gpu.EXTEND_PER_RAY
    print("%s %s libm, %d records: persistent vs per-lane %s, vs flat list %s" % (
        name, libm, len(rays), same_result(a, b) or "equal", same_result(a, c) or "equal"))
    assert same_result(a, b) == {} and same_result(a, c) == {}
    assert ((a.entries() + a.wrote()) == 1).all() and a.survivors == int(a.entries().sum())


# ------------------------------------------------------------------ fused
#: the fused runs: (scene, first depth, records).  curve_mix (open towards the camera, every material) from depth 1 to
#: the paths' ends; curves_small (a closed room but for its front: paths live long, and each of the test's rounds is
#: a launch) from kMaxDepth - 8, so that the kernel's own depth cap ends the paths that are left
FUSED_RUNS = {"curve_mix": (1, 1024), "curves_small": (sc.KMAX - 8, 1024)}


@pytest.mark.parametrize("libm", ["exact", "device"])
@pytest.mark.parametrize("name", list(FUSED_RUNS))
def test_fused_equals_iterated_steps(sched, oracle_mod, name, libm):
    """RT_STEP_FUSED (k_extend_curves<FUSE>: 3 the exact libm, 2 the device's) runs every record to its end: the
    colours are RT_STEP_STEP's, iterated by the test, bit for bit, and the launch's continuation segments the
    iteration's survivors.  Exact libm, throughput 1: orc_color_from within the frame gate, 0 records off by more
    than 1e-9.  That gate is an absolute one, made for a frame's radiances; a curve's normal is -d unnormalised, so a
    `scale` record (|d| = 2^40) onto a curve carries a radiance near 1e12, where neighbouring doubles lie 1.2e-4
    apart.  Where the oracle's colour exceeds 2^22 (spacing 9.3e-10, the gate itself) the records must agree to
    2^-40 of the colour instead: the forward and the backward product of a path of at most 100 segments differ by at
    most ~4 roundings a segment, 2^-44 of the colour, and 2^-40 is 16 times that; a defect (another hit) moves a
    colour by parts of itself.  FOUND by this test on an MI355X: 24 of curve_mix's 1024 records lie there; 12
    of them differ from orc_color_from, by at most 1.22e-4 absolute = 2.12e-16 of the colour (one spacing), all
    bit-equal to the iterated step, whose every round is orc_step's bit for bit; below 2^22 the largest deviation is
    1.14e-13."""
    sched.set_option("exact_libm", libm)
    depth, n = FUSED_RUNS[name]
    rays, ctr = cc.mixed(oracle_mod, name)
    pick = np.linspace(0, len(rays) - 1, n).astype(int)       # every class, not a prefix
    rays, ctr = rays[pick], ctr[pick]
    for unit in (False, True):
        T = np.ones((len(rays), 3)) if unit else sc.throughputs(len(rays), 1)
        f = step(cc.scene(name), rays, ctr, depth, T, mode=gpu.STEP_FUSED)
        assert f.extend == (gpu.EXTEND_CURVES_FUSED_EXACT if libm == "exact" else gpu.EXTEND_CURVES_FUSED)
        assert f.wrote().all() and not f.entries().any()
        want, segs = iterated(name, (libm, unit), rays, ctr, depth, T)
        same = sc.same_bits(f.color, want).all(axis=1)
        print("%s fused (%s libm, T %s): %d records, %d differ from the iterated step; segments %d / %d" % (
            name, libm, "1" if unit else "varied", len(rays), int((~same).sum()), f.survivors, segs))
        assert same.all(), (name, libm, np.flatnonzero(~same)[:4].tolist())
        assert f.survivors == segs
        if unit and libm == "exact":
            with np.errstate(all="ignore"):
                orc = cc.oracle_scene(oracle_mod, name).color_from(rays, depth, sc.SEED, sc.SMP, ctr_in=ctr)
                exact = sc.same_bits(f.color, orc).all(axis=1)
                big = np.abs(orc).max(axis=1) > 2.0 ** 22
                off = ~(np.abs(f.color - orc) <= 1e-9).all(axis=1) & ~exact & ~big
                rel = np.abs(f.color - orc).max(axis=1) / np.abs(orc).max(axis=1)
                off_big = big & ~exact & ~(rel <= 2.0 ** -40)
            print("%s fused vs orc_color_from: bit-exact share %.4f, off by more than 1e-9: %d; colours above 2^22: %d, "
                  "largest deviation there %.3e of the colour, off by more than 2^-40 of it: %d" % (
                      name, float(exact.mean()), int(off.sum()), int(big.sum()),
                      float(rel[big & ~exact].max()) if (big & ~exact).any() else 0.0, int(off_big.sum())))
            assert int(off.sum()) == 0 and int(off_big.sum()) == 0


@pytest.mark.parametrize("n", [64, 127, 128, 129, 2049])
def test_fused_ring_pressure(sched, oracle_mod, monkeypatch, n):
    """Records that all reach a hit within a few steps (`leave`, `inside`), one block: the four waves own every path,
    hits park by the dozen beside ready paths.  The rings hold kFuseRing = 256 entries against at most 127 owned
    paths (a wave claims new rays only with no ready path left: rt_device.h, FuseHit); the results are the unfused
    iteration's bit for bit."""
    rays, ctr = cc.quick_hits(oracle_mod, "curve_mix", n)
    T = sc.throughputs(n, 1)
    want, segs = iterate_steps(cc.scene("curve_mix"), rays, ctr, 1, T)
    monkeypatch.setenv("RTAMD_CURVE_BLOCKS", "1")
    f = step(cc.scene("curve_mix"), rays, ctr, 1, T, mode=gpu.STEP_FUSED)
    assert f.extend == gpu.EXTEND_CURVES_FUSED_EXACT and f.wrote().all()
    same = sc.same_bits(f.color, want).all(axis=1)
    print("ring pressure n %d: %d differ, segments %d / %d" % (n, int((~same).sum()), f.survivors, segs))
    assert same.all() and f.survivors == segs


# ------------------------------------------------------------------ tail
@pytest.mark.parametrize("name", ["curve_mix", "dup"])
def test_tail_equals_iterated_steps(sched, oracle_mod, name):
    """RT_STEP_TAIL (k_finish<kFeatCurves>, the per-lane curve test) on a curve-kernel scene: the iterated step's
    colours bit for bit, at depth 0 and 1."""
    rays, ctr = cc.mixed(oracle_mod, name, 512)
    for depth in (0, 1):
        T = sc.throughputs(len(rays), depth)
        tail = step(cc.scene(name), rays, ctr, depth, T, mode=gpu.STEP_TAIL)
        assert tail.wrote().all() and tail.finish is not None
        want = iterate_steps(cc.scene(name), rays, ctr, depth, T)[0] if depth == 0 else \
            iterated(name, ("exact", False, 512), rays, ctr, depth, T)[0]
        same = sc.same_bits(tail.color, want).all(axis=1)
        assert same.all(), (name, depth, int((~same).sum()), np.flatnonzero(~same)[:4].tolist())


# ------------------------------------------------------------------ the group path: one curve, the Klein set
@pytest.mark.parametrize("name", list(cc.GROUP_CASES))
def test_group_path_records(sched, oracle_mod, name):
    """A curve in a brute-force group, plain and under translate(rotate_y(...)) (its normal d * -1 formed on the
    local ray and taken back out of the chain), and the Kleinian set (klein_normal; the hit next to the surface
    just left): one step of k_extend<F> and the shades against orc_step, bit for bit."""
    sched.set_option("exact_libm", "exact")               # (Klein scenes hold no curve: their default is the device's)
    for cls, r in cc.records(oracle_mod, name).items():
        step_and_check(oracle_mod, name, r.rays, r.ctr, 1, cls, want_extend=gpu.EXTEND_PER_RAY)


# ------------------------------------------------------------------ refusals
def test_refusals(sched, oracle_mod, monkeypatch):
    rays, ctr = cc.mixed(oracle_mod, "curve_mix", 8)
    mix = cc.scene("curve_mix")
    with pytest.raises(RtError, match="depth >= 1"):
        gpu.step_rays(mix, rays, depth=0, mode=gpu.STEP_FUSED)
    with pytest.raises(RtError, match="unknown mode"):
        gpu.step_rays(mix, rays, depth=1, mode=3)
    with pytest.raises(RtError, match="unknown mode"):
        gpu.step_rays(mix, rays, depth=1, mode=-1)
    monkeypatch.setenv("RTAMD_CURVE_FUSE", "0")
    with pytest.raises(RtError, match="RTAMD_CURVE_FUSE=0"):
        gpu.step_rays(mix, rays, depth=1, mode=gpu.STEP_FUSED)
    monkeypatch.delenv("RTAMD_CURVE_FUSE")
    monkeypatch.setenv("RTAMD_CURVE_BLOCKS", "0")
    with pytest.raises(RtError, match="RTAMD_CURVE_BLOCKS=0"):
        gpu.step_rays(mix, rays, depth=1, mode=gpu.STEP_FUSED)
    monkeypatch.delenv("RTAMD_CURVE_BLOCKS")
    with pytest.raises(RtError, match="persistent curve kernel"):           # no curve-kernel scene: one curve in a group
        gpu.step_rays(cc.scene("cornell_bezier"), rays, depth=1, mode=gpu.STEP_FUSED)
    with pytest.raises(RtError, match="Perlin"):
        gpu.step_rays(_curves_with(perlin=True), rays, depth=1, mode=gpu.STEP_FUSED)
    with pytest.raises(RtError, match="samples a light"):
        gpu.step_rays(_curves_with(light=True), rays, depth=1, mode=gpu.STEP_FUSED)
    # the same scenes step and finish unfused
    for s in (_curves_with(perlin=True), _curves_with(light=True)):
        r = gpu.step_rays(s, rays, depth=1, seed=sc.SEED, smp=sc.SMP)
        assert r.extend == gpu.EXTEND_CURVES and ((r.entries() + r.wrote()) == 1).all()
    r = gpu.step_rays(mix, np.zeros((0, 7)), depth=1, mode=gpu.STEP_FUSED)
    assert r.color.shape == (0, 3) and r.survivors == 0


_variants = {}


def _curves_with(perlin=False, light=False):
    """A small curve-kernel scene with a noise-textured wall or a sampled light."""
    from rtamd import perlin as _perlin
    from rtamd import scene as g
    from rtamd import scenes
    from rtamd import vec as v
    key = (perlin, light)
    if key not in _variants:
        white = g.make_lambertian(g.constant_texture(v.vec3(0.73, 0.73, 0.73)))
        wall = g.make_lambertian(g.noise_texture(0.1)) if perlin else white
        lamp = g.flip_normals(g.make_xz_rect(213, 343, 227, 332, 554, g.make_diffuse_light(g.constant_texture(v.vec3(4, 4, 4)))))
        objs = [g.make_xz_rect(0, 555, 0, 555, 0, wall), lamp,
                g.make_bvh_node([g.bezier_array(scenes.random_polyline_curves(600), 3.0, white)], 0, 0)]
        _variants[key] = g.make_scene(objs, scenes.cornell_camera_for(cc.NX, cc.NY), g.sky_color,
                                      perlin=_perlin.from_seed(scenes.PERLIN_SEED) if perlin else None,
                                      light=lamp if light else None)
    return _variants[key]
