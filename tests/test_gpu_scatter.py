"""One scatter step of every shade kernel, record by record, against the oracle (tests/scatter_cases.py).

rt_step_rays runs one wavefront iteration (the render's extend launch, then launch_shade per material) on path
states the test chooses; the oracle's orc_step performs the same segment.  With the exact libm
(RT_OPT_EXACT_LIBM = exact) every field must be the same double: the hit's t and material, the survivor's origin,
direction, throughput and counter, the written colour; every record ends exactly one way (one survivor entry or
one sample write) and the device's survivor counters add up to the surviving records.

Not compared bit for bit, with the reason:
  - point records (the SOLO LDS extend's lambertian queue) carry no t: rt_step_rays reports NaN there, and the
    test checks the material and everything downstream instead;
  - with the device libm (RT_LIBM_DEVICE) the lambertian direction and throughput follow OCML's sin / cos, and
    the light branch of a sphere light follows them too (origin, counter, hit, status stay exact): bounded by
    DEVICE_LIBM_BOUND against the oracle, see test_device_libm;
  - a scatter inside a constant medium.  Its distance is neg_inv_density * log(next()) with the device library's
    log (rt_kernels.hip, the medium's hit test), which the project has not restated (RT_OPT_EXACT_LIBM covers sin
    and cos only).  FOUND BY THIS TEST on an MI355X: of the 80 media records one, scatter_cases.MEDIUM_LOG_RECORD
    (a vertical ray through the box medium), gets t = 3.6534284224434534 where the oracle (glibc's log) has
    3.653428422443453: one ulp, the same at depth 0 and 1; its hit / miss, material, draw counter, direction,
    throughput and status agree, and the origin follows t.  So a medium scatter's t and origin are compared as
    the device libm's lambertian vectors are: the largest deviation measured over the media class, relative to
    the oracle's t / the origin's largest component, asserted at 8 times (MEDIUM_T_BOUND, MEDIUM_ORIGIN_BOUND);
    everything else of the media class stays bit-exact.

The light list (LS = 2).  A one-element rt_set_light_list of a rect or a sphere commits as the single light
(rt_build.cpp light_records: LS = 1, not 2), so the list kernels are reached with a list naming the same rect
twice.  The oracle restates the header's list rule (orc_set_light_list: one index draw when m > 1, the sum of
(1 / m) * pdf_i), so these records are compared bit for bit like all others, and the list's tail with
orc_color_from.  On the panels the light's own plane ends most light-branch paths, so the room mix_two runs a
list of two different lights, a rect and a sphere, over points under, beside and behind them.
"""
import itertools

import numpy as np
import pytest

import scatter_cases as sc
from rtamd import gpu
from rtamd._lib import RtError

pytestmark = pytest.mark.gpu

HBM, LDS = gpu.STEP_EXTEND_HBM, gpu.STEP_EXTEND_LDS
# test_device_libm measures the largest deviation of a lambertian direction / throughput from the oracle with the
# device's sin / cos, relative to the vector's largest component, over the whole case set: 3.954e-16 on an MI355X
# (profiles/scatter_probe/report.txt).  8 times that: OCML's sin and cos are specified to about 1 ulp and the
# set is finite; the margin covers inputs not sampled, and is still orders of magnitude below any real defect.
DEVICE_LIBM_MEASURED = 3.954e-16
DEVICE_LIBM_BOUND = 8 * DEVICE_LIBM_MEASURED

# test_media_exact measures, over the media class at depth 0 and 1, the largest deviation of a medium scatter's t
# from the oracle's, relative to that t, and of the survivor's origin, relative to the oracle origin's largest
# component: 1.216e-16 and 3.298e-16 on an MI355X (one record, one ulp of t; profiles/scatter_probe/report.txt).
# Asserted at 8 times the measured maxima, as for the device libm: OCML's log is specified to about 1 ulp.
MEDIUM_T_MEASURED = 1.216e-16
MEDIUM_ORIGIN_MEASURED = 3.298e-16
MEDIUM_T_BOUND = 8 * MEDIUM_T_MEASURED
MEDIUM_ORIGIN_BOUND = 8 * MEDIUM_ORIGIN_MEASURED

_oracles = {}


def _oracle(oracle_mod, key):
    """The oracle's scene for a key: ("panel", noise, light: False / True (the single light) / "twice") or a room
    / solo name."""
    if key not in _oracles:
        if key[0] == "panel":
            _oracles[key] = sc.oracle_twin(oracle_mod, noise=key[1], light={False: None, True: "single"}.get(key[2], key[2]))
        elif key[0] == "solo":
            _oracles[key] = oracle_mod.build_scene(sc.solo_scene(*key[1:]))
        else:
            _oracles[key] = sc.oracle_room(oracle_mod, key[0])
    return _oracles[key]


_scenes = {}


def _panel(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _scenes:
        _scenes[key] = sc.panel_scene(**kw)
    return _scenes[key]


def _solo(n=24, noise=False):
    key = ("solo", n, noise)
    if key not in _scenes:
        _scenes[key] = sc.solo_scene(n, noise)
    return _scenes[key]


def _rel_dev(got, want):
    """per record: the largest componentwise deviation relative to the vector's largest component"""
    with np.errstate(all="ignore"):
        scale = np.max(np.abs(want), axis=1)
        d = np.max(np.abs(got - want), axis=1) / np.where(scale > 0, scale, 1.0)
    return np.where(sc.same_bits(got, want).all(axis=1), 0.0, np.where(np.isnan(d), np.inf, d))


def step_and_check(oracle_mod, scene, okey, rays, depth, ctr=None, extend=HBM, loose=None, tag="", medium_mats=()):
    """Run the step, compare with the oracle.  loose: records whose direction and throughput are bounded by
    DEVICE_LIBM_BOUND instead of bit-equal; medium_mats: the media's phase materials, whose hits' t and origin
    are bounded by MEDIUM_T_BOUND / MEDIUM_ORIGIN_BOUND.
    Returns (StepResult, Expect, the largest loose deviation, (the largest medium t, origin deviation))."""
    n = len(rays)
    T = sc.throughputs(n, depth)
    e = sc.expect(_oracle(oracle_mod, okey), rays, depth, T=T, ctr=ctr)
    r = gpu.step_rays(scene, rays, T_in=T, ctr_in=ctr, seed=sc.SEED, smp=sc.SMP, depth=depth, extend=extend)
    loose = np.zeros(n, dtype=bool) if loose is None else loose
    entries, wrote = r.entries(), r.wrote()
    ends = entries + wrote.astype(np.int32)
    bad = {}
    bad["ends exactly one way"] = ends != 1
    pt = np.zeros(n, dtype=bool)
    if r.shade.get(sc.MAT_LAMBERTIAN, (0, 0, 0, 0, False))[4]:
        pt = e.mtype == sc.MAT_LAMBERTIAN                      # point records: no t
        assert np.isnan(r.t[pt]).all()
    med = np.isin(e.mat, list(medium_mats))
    bad["hit t"] = ~sc.same_bits(r.t, e.t) & ~pt & ~med
    bad["hit material"] = r.mat != e.mat
    bad["survives"] = (entries == 1) != e.survive
    s = e.survive & (entries == 1)
    bad["survivor origin"] = ~sc.same_bits(r.ray[:, 0:3], e.ray[:, 0:3]).all(axis=1) & s & ~med
    bad["survivor counter"] = (r.ctr != e.ctr) & s
    exact = s & ~loose
    bad["survivor direction"] = ~sc.same_bits(r.ray[:, 3:6], e.ray[:, 3:6]).all(axis=1) & exact
    bad["survivor throughput"] = ~sc.same_bits(r.T, e.T).all(axis=1) & exact
    done = ~e.survive & wrote
    bad["colour"] = ~sc.same_bits(r.color, e.color).all(axis=1) & done
    med_dev = (0.0, 0.0)
    if med.any():
        with np.errstate(all="ignore"):
            dt = np.where(sc.same_bits(r.t, e.t), 0.0, np.abs(r.t - e.t) / np.abs(e.t))
            do = _rel_dev(r.ray[:, 0:3], e.ray[:, 0:3])
        ms = med & s
        med_dev = (float(dt[med].max()), float(do[ms].max()) if ms.any() else 0.0)
        bad["medium t"] = med & ~(dt <= MEDIUM_T_BOUND)
        bad["medium origin"] = ms & ~(do <= MEDIUM_ORIGIN_BOUND)
        print("%-34s depth %3d medium scatters %d: t differs on %d, largest %.3e of t; origin largest %.3e of its "
              "largest component" % (tag, depth, int(med.sum()), int((dt[med] > 0).sum()), med_dev[0], med_dev[1]))
    dev = 0.0
    lo = s & loose
    if lo.any():
        dd, dT = _rel_dev(r.ray[lo, 3:6], e.ray[lo, 3:6]), _rel_dev(r.T[lo], e.T[lo])
        dev = float(max(dd.max(), dT.max()))
        bad["loose direction"] = np.zeros(n, dtype=bool)
        bad["loose direction"][np.flatnonzero(lo)] = (dd > DEVICE_LIBM_BOUND) | (dT > DEVICE_LIBM_BOUND)
    print("%-34s depth %3d n %5d survive %5d wrote %5d loose %4d (max dev %.2e): %s" % (
        tag, depth, n, int(e.survive.sum()), int(wrote.sum()), int(lo.sum()), dev,
        ", ".join("%s %d" % (k, int(b.sum())) for k, b in bad.items() if b.any()) or "all equal"))
    for what, b in bad.items():
        k = np.flatnonzero(b)[:3]
        assert not b.any(), (tag, what, int(b.sum()), [(int(i), rays[i].tolist(), int(e.mtype[i])) for i in k])
    assert r.survivors == int(e.survive.sum()), (tag, r.survivors, int(e.survive.sum()))
    assert r.survivors == int(entries.sum())
    return r, e, dev, med_dev


def _exact(sched):
    sched.set_option("exact_libm", "exact")


# ------------------------------------------------------------------ (a) exact libm
@pytest.mark.parametrize("lit", [False, True])
@pytest.mark.parametrize("depth", [0, 1, sc.KMAX - 1, sc.KMAX])
def test_panel_classes_exact(sched, oracle_mod, depth, lit):
    """Every class of the panel scene, without and with the light mixture, at depth 0, 1, kMaxDepth - 1 and
    kMaxDepth (where only lights and the sky write anything but black)."""
    _exact(sched)
    scene = _panel(noise=True, light="single" if lit else None)
    for cls, rays in sc.panel_classes().items():
        step_and_check(oracle_mod, scene, ("panel", True, lit), rays, depth, tag="panel%s/%s" % ("+light" if lit else "", cls))
    if depth == 0:
        step_and_check(oracle_mod, scene, ("panel", True, lit), sc.recs_time(), 0, tag="panel/time")


@pytest.mark.parametrize("ctr0", range(8))
def test_counter_phases_exact(sched, oracle_mod, ctr0):
    """The same records from draw counter 0..7: the metal rejection loop, the dielectric's single draw and the
    lambertian's six start at every phase of the Philox block."""
    _exact(sched)
    rays = sc.mixed()
    ctr = (np.arange(len(rays), dtype=np.uint32) % 3) * 8 + ctr0          # not every record at the same counter
    for lit in (False, True):
        step_and_check(oracle_mod, _panel(noise=True, light="single" if lit else None), ("panel", True, lit), rays, 1,
                       ctr=ctr, tag="ctr %d%s" % (ctr0, " +light" if lit else ""))


@pytest.mark.parametrize("name", ["mix_rect", "mix_sphere", "mix_two"])
def test_light_mixture_exact(sched, oracle_mod, name):
    """Points under, beside (on its plane), behind and inside the light; the oracle ends the paths whose pdf is 0
    or NaN (tests/test_scatter_host.py shows the set holds them).  mix_two: a list of two different lights, a
    rect and a sphere (LS = 2), against the oracle's list rule."""
    _exact(sched)
    for depth in (0, 1):
        for ctr0 in (0, 1):
            rays = sc.recs_room_mixture()
            r = step_and_check(oracle_mod, sc.rooms()[name], (name,), rays, depth,
                               ctr=np.full(len(rays), ctr0, dtype=np.uint32), tag="%s ctr %d" % (name, ctr0))[0]
            assert r.shade[sc.MAT_LAMBERTIAN][1] == (2 if name == "mix_two" else 1)


@pytest.mark.parametrize("depth", [0, 1])
def test_media_exact(sched, oracle_mod, depth):
    """Rays through, into and past a box medium and a sphere medium: the medium's draws inside the hit test and
    the counter handed on to the shade."""
    _exact(sched)
    rays = sc.recs_media()
    r, e, _, md = step_and_check(oracle_mod, sc.rooms()["media"], ("media",), rays, depth, tag="media",
                                 medium_mats=sc.MEDIA_PHASE_MATS)
    print("media depth %d: medium t deviation %.3e (bound %.3e), origin %.3e (bound %.3e)" % (
        depth, md[0], MEDIUM_T_BOUND, md[1], MEDIUM_ORIGIN_BOUND))
    surface = ~np.isin(e.mat, list(sc.MEDIA_PHASE_MATS))
    assert set(e.mat[surface]) <= {-1, 0, 3} and (~surface).sum() >= 20        # floor, metal sphere, sky; the media
    k = sc.MEDIUM_LOG_RECORD
    assert np.array_equal(rays[k], [0.1 * 6 - 0.8, 5.0, 0.3, 0.0, -1.0, 0.0, 0.0]) and e.mat[k] == 1
    print("MEDIUM_LOG_RECORD depth %d: oracle t %r, device t %r" % (depth, float(e.t[k]), float(r.t[k])))


@pytest.mark.parametrize("n,noise", [(24, False), (24, True), (300, False)])
def test_solo_world_exact_both_extends(sched, oracle_mod, n, noise):
    """A one-BVH sphere world through k_extend and, at depth >= 1, through k_extend_lds with point records."""
    _exact(sched)
    scene, rays = _solo(n, noise), sc.recs_solo(n)
    step_and_check(oracle_mod, scene, ("solo", n, noise), rays, 0, tag="solo %d hbm" % n)
    step_and_check(oracle_mod, scene, ("solo", n, noise), rays, 1, tag="solo %d hbm" % n)
    r, _, _, _ = step_and_check(oracle_mod, scene, ("solo", n, noise), rays, 1, extend=LDS, tag="solo %d lds" % n)
    assert r.shade[sc.MAT_LAMBERTIAN][4] == gpu.point_hits(gpu.upload(scene))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2049])
def test_queue_shapes(sched, oracle_mod, n):
    """Prefixes of the mixed set around a wave, a block and (2049) more than eight blocks, so every shard is
    appended to; at kMaxDepth every metal, dielectric and lambertian record dies, and a set of dielectric records
    survives whole."""
    _exact(sched)
    scene = _panel(noise=True, light=None)
    rays = sc.mixed(n)
    r, e, _, _ = step_and_check(oracle_mod, scene, ("panel", True, False), rays, 1, tag="prefix %d" % n)
    assert r.status.shape == (n,)
    if n == 0:
        assert r.survivors == 0 and r.shade == {}
        return
    r, e, _, _ = step_and_check(oracle_mod, scene, ("panel", True, False), rays, sc.KMAX, tag="prefix %d, all die" % n)
    assert r.survivors == 0 and r.wrote().all()
    glass = np.tile(sc.recs_critical(), (n // 50 + 1, 1))[:n]
    r, e, _, _ = step_and_check(oracle_mod, scene, ("panel", True, False), glass, 1, tag="prefix %d, all survive" % n)
    assert r.survivors == n and not r.wrote().any()


# ------------------------------------------------------------------ (b) device libm
def _device_runs(oracle_mod):
    """The case set with the device's sin / cos: (tag, StepResult, Expect, deviation) per run."""
    out = []
    for lit in (False, True):
        scene = _panel(noise=True, light="single" if lit else None)
        for depth in (0, 1):
            for cls, rays in sc.panel_classes().items():
                e0 = sc.expect(_oracle(oracle_mod, ("panel", True, lit)), rays, depth)
                out.append(step_and_check(oracle_mod, scene, ("panel", True, lit), rays, depth,
                                          loose=e0.mtype == sc.MAT_LAMBERTIAN, tag="device panel%s/%s" % ("+light" if lit else "", cls)))
    for name in ("mix_rect", "mix_sphere", "mix_two"):
        rays = sc.recs_room_mixture()
        e0 = sc.expect(_oracle(oracle_mod, (name,)), rays, 1)
        out.append(step_and_check(oracle_mod, sc.rooms()[name], (name,), rays, 1, loose=e0.mtype == sc.MAT_LAMBERTIAN,
                                  tag="device " + name))
    return out


def test_device_libm(sched, oracle_mod):
    """RT_LIBM_DEVICE: hit, the survivor's origin, the counter, the status, metal, dielectric and lights stay
    bit-exact; the lambertian direction and throughput stay within DEVICE_LIBM_BOUND of the oracle."""
    sched.set_option("exact_libm", "device")
    runs = _device_runs(oracle_mod)
    worst = max(run[2] for run in runs)
    print("device libm: largest lambertian deviation from the oracle %.3e (bound %.3e)" % (worst, DEVICE_LIBM_BOUND))
    assert worst <= DEVICE_LIBM_BOUND


# ------------------------------------------------------------------ (c) every instance
# k_shade<MAT, TL, LS, LL, EX, PT> as shade_kernel can return them, written out (TL: 0 plain, 1 Perlin, 2 image)
LAMBERTIAN = {(0,) + t + (False,) for t in itertools.product((0, 1, 2), (0, 1, 2), (False, True), (False, True))}
LAMBERTIAN_PT = {(0, tl, 0, ll, ex, True) for tl in (0, 1) for ll in (False, True) for ex in (False, True)}
METAL = {(1, tl, 0, ll, False, False) for tl in (0, 1, 2) for ll in (False, True)}
DIELECTRIC = {(2, 0, 0, ll, False, False) for ll in (False, True)}
LIGHT = {(3, tl, 0, ll, False, False) for tl in (0, 1, 2) for ll in (False, True)}
ALL_SHADE = LAMBERTIAN | LAMBERTIAN_PT | METAL | DIELECTRIC | LIGHT
assert len(ALL_SHADE) == 36 + 8 + 6 + 2 + 6
UNREACHABLE = set()            # none: every instance shade_kernel can return is run below

def _run_guarded(results, key, fn):
    """fn() under its key: its return value, or the assertion that stopped it (raised again by the test of that key)"""
    try:
        results[key] = (fn(), None)
    except AssertionError as err:
        results[key] = (set(), err)


def _panel_instances(oracle_mod, tex, libm):
    """The mixed set through the instances of one texture level and libm mode: LS 0 / 1 / 2 (no light, the single
    light, the list naming it twice) x the leaf records in LDS or not (300 far spheres).  The decoys are out of
    every ray's reach, so the expectation is the oracle's step on the scene without them."""
    reached = set()
    rays = sc.mixed()
    noise = tex != "plain"
    for light in (None, "single", "twice"):
        okey = ("panel", noise, light or False)
        lam = sc.expect(_oracle(oracle_mod, okey), rays, 1).mtype == sc.MAT_LAMBERTIAN
        for many in (False, True):
            scene = _panel(noise=noise, light=light, image=tex == "image", many=many, tri=many and tex == "image")
            r = step_and_check(oracle_mod, scene, okey, rays, 1, loose=lam if libm == "device" else None,
                               tag="%s %s light=%s many=%d" % (tex, libm, light, many))[0]
            want = ({"plain": 0, "perlin": 1, "image": 2}[tex], {None: 0, "single": 1, "twice": 2}[light], not many,
                    libm == "exact", False)
            assert r.shade[sc.MAT_LAMBERTIAN] == want, (r.shade, want)
            reached |= {(m,) + tuple(t) for m, t in r.shade.items()}
    return reached


def _point_record_instances(oracle_mod, libm):
    reached = set()
    for n, noise in ((24, False), (24, True), (300, False), (300, True)):
        scene, rays = _solo(n, noise), sc.recs_solo(n)
        lam = sc.expect(_oracle(oracle_mod, ("solo", n, noise)), rays, 1).mtype == sc.MAT_LAMBERTIAN
        r = step_and_check(oracle_mod, scene, ("solo", n, noise), rays, 1, extend=LDS,
                           loose=lam if libm == "device" else None, tag="solo %d noise=%d %s" % (n, noise, libm))[0]
        assert r.shade[sc.MAT_LAMBERTIAN] == (1 if noise else 0, 0, n <= 256, libm == "exact", True), r.shade
        reached |= {(m,) + tuple(t) for m, t in r.shade.items()}
    return reached


@pytest.fixture(scope="module")
def shade_sweep(gpu_ctx, oracle_mod):
    """Every instance run of (c), once per module: {(tex or "points", libm): (instances launched, failure)}."""
    out = {}
    try:
        for libm in ("exact", "device"):
            gpu_ctx.set_option("exact_libm", libm)
            for tex in ("plain", "perlin", "image"):
                _run_guarded(out, (tex, libm), lambda: _panel_instances(oracle_mod, tex, libm))
            _run_guarded(out, ("points", libm), lambda: _point_record_instances(oracle_mod, libm))
    finally:
        gpu_ctx.reset_options()
    return out


@pytest.mark.parametrize("libm", ["exact", "device"])
@pytest.mark.parametrize("tex", ["plain", "perlin", "image", "points"])
def test_every_instance(shade_sweep, tex, libm):
    """One texture level (or the point-record instances of the SOLO worlds) in one libm mode: see _panel_instances
    and _point_record_instances."""
    reached, err = shade_sweep[(tex, libm)]
    if err is not None:
        raise err
    assert reached


def test_union_of_instances_is_the_enumeration(shade_sweep):
    """What the sweep launched is every instance of the enumeration, and nothing else."""
    reached = set().union(*(r for r, _ in shade_sweep.values()))
    missing, extra = ALL_SHADE - UNREACHABLE - reached, reached - ALL_SHADE
    print("k_shade instances reached: %d of %d" % (len(reached & ALL_SHADE), len(ALL_SHADE)))
    for t in sorted(reached):
        print("  k_shade<mat %d, TL %d, LS %d, LL %d, EX %d, PT %d>" % tuple(int(x) for x in t))
    assert not missing and not extra, (sorted(missing), sorted(extra))


# ------------------------------------------------------------------ (d) the tail
def iterate_steps(scene, rays, depth=0):
    """STEP mode iterated to the end: each round's survivors go back in at depth + 1 with their throughput,
    counter and pixel key; at most kMaxDepth + 2 rounds.  Returns the colours (n, 3)."""
    n = len(rays)
    out = np.full((n, 3), np.nan)
    done = np.zeros(n, dtype=bool)
    cur, T, ctr, pix = rays.copy(), sc.throughputs(n, depth), np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)
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
        cur = np.concatenate([r.ray[s], np.zeros((int(s.sum()), 1))], axis=1)
        T, ctr, pix = r.T[s], r.ctr[s], pix[s]
    assert len(cur) == 0 and done.all()
    return out


TAILS = {
    # name: (scene, oracle key, libm)
    "panel": (lambda: _panel(noise=True, light=None), ("panel", True, False), "exact"),
    "panel_lit_device": (lambda: _panel(noise=False, light="single"), ("panel", False, True), "device"),
    "panel_image_list": (lambda: _panel(noise=True, light="twice", image=True, many=True, tri=True),
                         ("panel", True, "twice"), "exact"),
    "solo": (lambda: _solo(24, False), ("solo", 24, False), "exact"),
    "solo_noise_device": (lambda: _solo(24, True), ("solo", 24, True), "device"),
}


def _tail_run(oracle_mod, name):
    """k_finish against the iterated steps (bit for bit, depth 0 and 1) and, at depth 0, where the throughput is 1
    and the oracle's colour is the path's, against orc_color_from within the frame gate.  Returns the instances."""
    make, okey, _ = TAILS[name]
    scene = make()
    rays = (sc.recs_solo(24) if name.startswith("solo") else sc.mixed())[:512]
    n = len(rays)
    inst = set()
    for depth in (0, 1):
        T = sc.throughputs(n, depth)
        tail = gpu.step_rays(scene, rays, T_in=T, seed=sc.SEED, smp=sc.SMP, depth=depth, mode=gpu.STEP_TAIL)
        assert tail.wrote().all()
        inst.add(tail.finish)
        steps = iterate_steps(scene, rays, depth)
        same = sc.same_bits(tail.color, steps).all(axis=1)
        assert same.all(), (name, depth, int((~same).sum()), np.flatnonzero(~same)[:4].tolist())
        if depth != 0:
            continue
        with np.errstate(all="ignore"):
            want = _oracle(oracle_mod, okey).color_from(rays, 0, sc.SEED, sc.SMP)
            exact = sc.same_bits(tail.color, want).all(axis=1)
            off = ~(np.abs(tail.color - want) <= 1e-9).all(axis=1) & ~exact
        print("%s: tail vs orc_color_from, %d records: bit-exact share %.4f, off by more than 1e-9: %d" % (
            name, n, float(exact.mean()), int(off.sum())))
        assert int(off.sum()) <= n // 200, (name, int(off.sum()))
    return inst


@pytest.fixture(scope="module")
def tail_sweep(gpu_ctx, oracle_mod):
    """Every tail run, once per module: {name: (k_finish instances launched, failure)}."""
    out = {}
    try:
        for name, (_, _, libm) in TAILS.items():
            gpu_ctx.set_option("exact_libm", libm)
            _run_guarded(out, name, lambda: _tail_run(oracle_mod, name))
    finally:
        gpu_ctx.reset_options()
    return out


@pytest.mark.parametrize("name", list(TAILS))
def test_tail_equals_iterated_steps(tail_sweep, name):
    """k_finish's colours are the STEP mode's, iterated by the test, bit for bit; and the oracle's color() from
    the same states within test_scene_parity's gate (at most n // 200 records off by more than 1e-9)."""
    inst, err = tail_sweep[name]
    if err is not None:
        raise err
    assert inst


def test_tail_instances_cover_the_axes(tail_sweep):
    inst = set().union(*(i for i, _ in tail_sweep.values()))
    for t in sorted(inst):
        print("  k_finish<F %d, TL %d, LS %d, SOLO %d, EX %d>" % tuple(int(x) for x in t))
    assert {t[2] for t in inst} == {0, 1, 2}
    assert {t[1] for t in inst} == {0, 1, 2}
    assert {t[4] for t in inst} == {False, True}
    assert {t[3] for t in inst} == {False, True}


# ------------------------------------------------------------------ (e) refusals
def test_refusals(sched):
    import ctypes
    from rtamd import _lib, scenes
    scene = _panel(noise=True, light=None)
    rays = sc.mixed()[:8]
    with pytest.raises(RtError, match="depth outside"):
        gpu.step_rays(scene, rays, depth=-1)
    with pytest.raises(RtError, match="depth outside"):
        gpu.step_rays(scene, rays, depth=sc.KMAX + 1)
    with pytest.raises(RtError, match="unknown extend"):
        gpu.step_rays(scene, rays, extend=2)
    with pytest.raises(RtError, match="unknown mode"):
        gpu.step_rays(scene, rays, mode=3)
    with pytest.raises(RtError, match="would not take the fused curve extend"):     # RT_STEP_FUSED: curve-kernel scenes only
        gpu.step_rays(scene, rays, depth=1, mode=gpu.STEP_FUSED)
    with pytest.raises(RtError, match="throughput 1"):
        gpu.step_rays(scene, rays, T_in=np.full((8, 3), 0.5), depth=0)
    bad = rays.copy()
    bad[3, 6] = 0.5
    with pytest.raises(RtError, match=r"time \+0\.0 \(record 3"):
        gpu.step_rays(scene, bad, depth=1)
    bad[3, 6] = -0.0
    with pytest.raises(RtError, match=r"time \+0\.0 \(record 3"):
        gpu.step_rays(scene, bad, depth=1)
    with pytest.raises(RtError, match="LDS"):                       # a generic tree has no LDS extend
        gpu.step_rays(scene, rays, depth=1, extend=LDS)
    with pytest.raises(RtError, match="depth >= 1"):
        gpu.step_rays(_solo(), sc.recs_solo()[:8], depth=0, extend=LDS)
    # scenes whose renders take the persistent curve kernel are stepped through it (tests/test_gpu_curve_step.py)
    r = gpu.step_rays(scenes.cornell_curves_small(16, 16), rays, depth=1)
    assert r.extend == gpu.EXTEND_CURVES and ((r.entries() + r.wrote()) == 1).all()
    assert gpu.step_rays(scene, rays, depth=1).extend == gpu.EXTEND_PER_RAY
    # null pointers, n < 0, an uncommitted scene: through the ABI itself
    h = gpu.upload(scene)
    L = _lib.lib()
    dp, ip, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    d = (ctypes.c_double * 64)()
    i = (ctypes.c_int32 * 64)()
    u = (ctypes.c_uint32 * 64)()
    args = [h, 1, d, d, u, None, ctypes.c_uint64(1), ctypes.c_uint32(0), 1, 0, 0, i, d, d, d, u, d, i, i, u]
    for k in (2, 3, 4, 11, 12, 13, 14, 15, 16, 17, 18, 19):
        a = list(args)
        a[k] = None
        assert L.rt_step_rays(*a) != 0 and b"null pointer" in L.rt_last_error(), k
    a = list(args)
    a[1] = -1
    assert L.rt_step_rays(*a) != 0 and b"must be >= 0" in L.rt_last_error()
    b = gpu.GpuBuilder(sched)
    a = list(args)
    a[0] = b.scene
    assert L.rt_step_rays(*a) != 0 and b"not committed" in L.rt_last_error()
    r = gpu.step_rays(scene, np.zeros((0, 7)), depth=1)
    assert r.status.shape == (0,) and r.survivors == 0 and r.shade == {}
    r = gpu.step_rays(scene, np.zeros((0, 7)), depth=1, mode=gpu.STEP_TAIL)
    assert r.color.shape == (0, 3) and r.finish is None
