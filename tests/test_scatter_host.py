"""The scatter cases against the oracle alone (no GPU): every class of tests/scatter_cases.py reaches the branch
it is named for, orc_step iterated to the end is orc_color_from, and orc_color_from started from a sample's
camera state is orc_sample.  What the GPU tests compare with rt_step_rays is therefore not vacuous."""
import math

import numpy as np
import pytest

import scatter_cases as sc
from rtamd import scenes

KIND, HIT, T, MAT, MTYPE = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def panel(oracle_mod):
    return sc.oracle_twin(oracle_mod, noise=True, light=None)


@pytest.fixture(scope="module")
def panel_lit(oracle_mod):
    return sc.oracle_twin(oracle_mod, noise=True, light="single")


def _rows(osc, rays, depth=1, ctr=None):
    with np.errstate(all="ignore"):
        return osc.step(rays, depth, sc.SEED, sc.SMP, ctr_in=ctr)[0]


def test_exact_hit_points(panel, oracle_mod):
    """The vertical rays land on the coordinates the classes name, bit for bit, at t = 2."""
    xs = sc.checker_points()
    R = sc.Recs()
    for x in xs:
        R.down(x, 0.25)
    rows = _rows(panel, R.done())
    assert (rows[:, HIT] == 1).all() and (rows[:, T] == 2.0).all()
    assert sc.same_bits(rows[:, 18], np.array(xs)).all()
    assert (rows[:, 19] == 1.0).all() and (rows[:, 20] == 0.25).all()


def test_checker_class_sits_on_the_sines_zeros(panel):
    rows = _rows(panel, sc.panel_classes()["checker"])
    assert (rows[:, HIT] == 1).all()
    p = rows[:, 18:21]
    prod = np.sin(10 * p[:, 0]) * np.sin(10 * p[:, 1]) * np.sin(10 * p[:, 2])
    near = np.abs(prod) < 1e-12
    assert near.sum() >= 20, int(near.sum())
    assert (prod[near] > 0).any() and (prod[near] < 0).any()      # either side of the zeros
    assert (np.abs(10 * p[:, 0]) >= 2.0 ** 20).sum() >= 6
    assert (p[:, 1] != 0).all()                       # never the plane y = 0


def test_noise_class_reaches_lattice_points_and_wraps(panel):
    rows = _rows(panel, sc.panel_classes()["noise"])
    assert (rows[:, HIT] == 1).all()
    q = rows[:, 18] * 4.0                              # the scale-4 panels' p * scale
    on_noise = np.abs(rows[:, 20] - sc.panel_z("noise")) <= 1.0
    qs = q[on_noise]
    for want in (0.0, 255.0, 256.0, -1.0, -256.0):
        assert (qs == want).any(), want
        assert ((qs < want) & (want - qs <= 1e-12 * max(1.0, abs(want)))).any(), want      # just below it
    assert (np.floor(qs) < 0).any()
    assert (np.abs(rows[:, 20]) >= 2.0 ** 20 - 1).sum() >= 3     # marble with large |z|
    assert (rows[:, 19] > 5).sum() >= 10                         # the spheres


def test_onb_class_straddles_the_switch(panel):
    rows = _rows(panel, sc.panel_classes()["onb"])
    n = rows[:, 21:24][rows[:, HIT] == 1]
    unit_x = np.abs(n[:, 0] / np.sqrt((n * n).sum(axis=1)))
    assert (unit_x > 0.9).sum() >= 8 and ((unit_x <= 0.9) & (unit_x > 0.89)).sum() >= 8
    assert (np.abs(n[:, 0]) == 0.9).any()
    for axis in range(3):
        for sign in (1.0, -1.0):
            e = np.zeros(3)
            e[axis] = sign
            assert (n == e).all(axis=1).any(), (axis, sign)


def test_metal_class_has_absorbed_and_surviving(panel):
    rays = sc.panel_classes()["metal"]
    for ctr0 in range(8):
        rows = _rows(panel, rays, ctr=np.full(len(rays), ctr0, dtype=np.uint32))
        assert (rows[:, MTYPE] == sc.MAT_METAL).all()
        assert (rows[:, KIND] == 1).sum() >= 20 and (rows[:, KIND] == 0).sum() >= 5, ctr0


def test_dielectric_sweep_straddles_the_critical_angle(panel):
    rays = sc.recs_critical()
    rows = _rows(panel, rays)
    assert (rows[:, MTYPE] == sc.MAT_DIELECTRIC).all() and (rows[:, KIND] == 1).all()
    sin_a = rays[:, 3] / np.hypot(rays[:, 3], rays[:, 4])
    refracted = rows[:, 12] > 0                        # goes on upward; a reflection comes back down
    below, above = sin_a < 1 / 1.5 - 1e-12, sin_a > 1 / 1.5 + 1e-12
    assert refracted[below].any() and not refracted[above].any()
    assert below.sum() >= 8 and above.sum() >= 8
    close = np.abs(sin_a - 1 / 1.5) < 1e-14           # the ulp steps: both outcomes among them
    assert refracted[close].any() and (~refracted[close]).any()


def test_mixture_classes_hold_ended_paths(panel_lit, oracle_mod):
    rows = _rows(panel_lit, sc.panel_classes()["mixture"])
    lam = rows[:, MTYPE] == sc.MAT_LAMBERTIAN
    assert lam.all()
    assert (rows[:, KIND] == 0).sum() >= 8 and (rows[:, KIND] == 1).sum() >= 8
    for name in ("mix_rect", "mix_sphere"):
        o = oracle_mod.build_scene(sc.rooms()[name])
        r = _rows(o, sc.recs_room_mixture())
        lam = r[:, MTYPE] == sc.MAT_LAMBERTIAN
        assert lam.sum() >= 24, name
        assert ((r[:, KIND] == 0) & lam).sum() >= 5 and ((r[:, KIND] == 1) & lam).sum() >= 10, name


def test_oracle_light_list_rule(panel_lit, oracle_mod):
    """orc_set_light_list with one light named twice (include/rt.h, "light lists"): the density is the single
    light's (0.5 p + 0.5 p), so a record on the mixture's cosine branch is the single light's bit for bit; the
    light branch draws the index first, one number more, and lands on the light all the same."""
    twice = sc.oracle_twin(oracle_mod, noise=True, light="twice")
    rays = np.concatenate([sc.panel_classes()["mixture"], sc.panel_classes()["checker"]])
    with np.errstate(all="ignore"):
        r1, c1 = panel_lit.step(rays, 1, sc.SEED, sc.SMP)
        r2, c2 = twice.step(rays, 1, sc.SEED, sc.SMP)
    lam = r1[:, MTYPE] == sc.MAT_LAMBERTIAN
    first = np.array([oracle_mod.stream(sc.SEED, k, sc.SMP, 0, 1)[0] for k in range(len(rays))])
    cosine, light = lam & (first >= 0.5), lam & (first < 0.5)
    assert cosine.sum() >= 20 and light.sum() >= 20
    assert sc.same_bits(r1[~light], r2[~light]).all() and (c1[~light] == c2[~light]).all()
    assert (c2[light] == c1[light] + 1).all() and (c1[light] == 3).all()
    # two different lights (the room mix_two): both are sampled, each record's scattered ray points at the one
    # its index draw names, and paths survive and end on the light branch
    two = sc.oracle_room(oracle_mod, "mix_two")
    rays = sc.recs_room_mixture()
    n_rect = n_sphere = n_on = n_ended = 0
    for c0 in (0, 1):                                   # the GPU test's two counter phases
        with np.errstate(all="ignore"):
            rows, ctr = two.step(rays, 1, sc.SEED, sc.SMP, ctr_in=np.full(len(rays), c0, dtype=np.uint32))
        s1 = np.array([oracle_mod.stream(sc.SEED, k, sc.SMP, c0, 2) for k in range(len(rays))])
        lam = rows[:, MTYPE] == sc.MAT_LAMBERTIAN
        light = lam & (s1[:, 0] < 0.5)
        to_rect, to_sphere = light & (s1[:, 1] < 0.5), light & (s1[:, 1] >= 0.5)
        assert (ctr[to_rect] == c0 + 4).all() and (ctr[to_sphere] == c0 + 8).all()   # choice, index, then 2 or 6 draws
        sv = to_rect & (rows[:, KIND] == 1)
        aim = rows[sv, 18:21] + rows[sv, 11:14]
        assert (np.abs(aim[:, 1] - 4.0) < 1e-9).all() and (np.abs(aim[:, 0]) <= 1 + 1e-9).all()
        n_rect, n_sphere = n_rect + int(to_rect.sum()), n_sphere + int(to_sphere.sum())
        n_on, n_ended = n_on + int(((rows[:, KIND] == 1) & light).sum()), n_ended + int(((rows[:, KIND] == 0) & light).sum())
    assert n_rect >= 10 and n_sphere >= 10 and n_on >= 16 and n_ended >= 2, (n_rect, n_sphere, n_on, n_ended)
    with pytest.raises(ValueError):
        two.set_light_list([])


def test_media_class_draws_inside_the_hit_test(oracle_mod):
    o = oracle_mod.build_scene(sc.rooms()["media"])
    rays = sc.recs_media()
    with np.errstate(all="ignore"):
        rows, ctr = o.step(rays, 1, sc.SEED, sc.SMP)
    assert (rows[:, HIT] == 0).any() and (rows[:, HIT] == 1).any()
    assert (rows[:, MTYPE] == sc.MAT_LAMBERTIAN).sum() >= 10
    assert (ctr[rows[:, HIT] == 0] > 0).any()          # a miss that drew: the medium's own draw


@pytest.mark.parametrize("depth", [0, 1, sc.KMAX - 1, sc.KMAX])
def test_step_iterated_equals_color_from(panel, panel_lit, depth):
    rays = sc.mixed()[::3]
    for osc in (panel, panel_lit):
        with np.errstate(all="ignore"):
            want = osc.color_from(rays, depth, sc.SEED, sc.SMP)
        got = sc.iterate_oracle(osc, rays, depth)
        assert sc.same_bits(got, want).all()


def test_color_from_camera_state_equals_sample(oracle_mod):
    """orc_trace_sample records the camera ray, and its counter only after the first hit test (which draws in
    scenes with media), so the ray's time and the counter before that test are recovered from the sample's own
    stream by get-ray's draw pattern (_camera_state), with the shutter read from the scene's camera.  A wrong
    recovery cannot pass: the colour must be orc_sample's bit for bit."""
    nx, ny, seed = 24, 16, 0x5EED0402
    for make in (scenes.random_scene, scenes.cornell_box, scenes.cornell_smoke):
        scene = make(nx, ny)
        o = oracle_mod.build_scene(scene)
        for (x, y, smp) in ((0, 0, 0), (5, 7, 1), (23, 15, 2), (11, 3, 5), (12, 9, 0)):
            tr = o.trace_sample(nx, ny, x, y, seed, smp, cap=1)
            want = np.array(o.sample(nx, ny, x, y, seed, smp))
            ray, ctr = _camera_state(scene, oracle_mod, nx, ny, x, y, seed, smp, tr[0])
            got = o.color_from(ray[None, :], 0, seed, smp, pix=[y * nx + x], ctr_in=[ctr])[0]
            assert sc.same_bits(got, want).all(), (make.__name__, x, y, smp)


def _camera_state(scene, oracle_mod, nx, ny, x, y, seed, smp, first):
    """The camera ray (from the trace's first segment) with its time and draw counter: trace-all draws the two
    jitters, get-ray disk points until one lies in the unit disk (whatever the aperture), then the time
    t0 + r (t1 - t0) from the camera's shutter slots (camera.scm:80-92)."""
    t0, t1 = scene.camera.slots()[22:24]
    pixk = y * nx + x
    s = oracle_mod.stream(seed, pixk, smp, 0, 64)
    k = 2
    while True:
        a, b = s[k] * 2 - 1, s[k + 1] * 2 - 1
        k += 2
        if a * a + b * b < 1.0:
            break
    tm = t0 + s[k] * (t1 - t0)
    return np.array(list(first[0:6]) + [tm]), k + 1
