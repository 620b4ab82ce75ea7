"""The curve step cases against the oracle alone (no GPU): every new class of tests/curve_step_cases.py meets the
curve the way it is named, orc_step iterated to the end is orc_color_from on these records, and the records are
ones the curve kernel may be given.  What tests/test_gpu_curve_step.py compares is therefore not vacuous."""
import numpy as np
import pytest

import curve_step_cases as cc
import hit_ray_cases as hc
import scatter_cases as sc

KIND, HIT, T, MAT = 0, 1, 2, 3


def _rows(oracle_mod, name, recs, depth=1):
    with np.errstate(all="ignore"):
        return cc.oracle_scene(oracle_mod, name).step(recs.rays, depth, sc.SEED, sc.SMP, ctr_in=recs.ctr)[0]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_new_classes_hit_curves(oracle_mod, name):
    """In every new class of a curve-kernel scene the closest hit is a curve (normal = -d bit for bit) on at least a
    quarter of the records, and at least a tenth end otherwise (a wall, a sphere, the sky)."""
    recs = cc.records(oracle_mod, name)
    assert set(cc.CASES[name][1]) | set(cc.CASES[name][2]) == set(recs)
    for cls in cc.CASES[name][2]:
        r = recs[cls]
        rows = _rows(oracle_mod, name, r, 0 if cls == "moving" else 1)
        on = cc.curve_hit(rows, r.rays)
        print("%-14s %-9s records %d: curve hits %d, other hits %d, misses %d" % (
            name, cls, len(r), int(on.sum()), int(((rows[:, HIT] == 1) & ~on).sum()), int((rows[:, HIT] == 0).sum())))
        assert len(r) == cc.N
        assert on.sum() >= len(r) // 4, (name, cls, int(on.sum()))
        assert (~on).sum() * 10 >= len(r), (name, cls, int((~on).sum()))


def test_old_classes_are_hit_ray_cases_own(oracle_mod):
    """The hit_ray_cases classes are taken as they are: curves_small's are that module's rays bit for bit, and the
    oracle's curve hits on them are the few the classes reach (the reason for the new ones)."""
    _, rays = hc.scene_rays("curves_small", *hc.CASES["curves_small"][:2])
    recs = cc.records(oracle_mod, "curves_small")
    counts = {}
    for cls in hc._CURVE_CLASSES:
        assert np.array_equal(recs[cls].rays, rays[cls][0])
        counts[cls] = int(cc.curve_hit(_rows(oracle_mod, "curves_small", recs[cls]), recs[cls].rays).sum())
    print("curves_small, curve hits per hit_ray_cases class:", counts)
    assert counts["plane"] < 16 and counts["surface"] < 16 and counts["tangent"] > 128


def test_dup_class_holds_exact_ties(oracle_mod):
    """A hit on the second or third copy of a curve is a tie in z with the first: at least a quarter of `dup`."""
    r = cc.records(oracle_mod, "dup")["dup"]
    rows = _rows(oracle_mod, "dup", r)
    on = cc.curve_hit(rows, r.rays)
    tie = on & np.isin(rows[:, MAT], (cc.DUP_SECOND, cc.DUP_THIRD))
    first = on & (rows[:, MAT] == cc.DUP_FIRST)
    print("dup: curve hits %d, ties to a later copy %d, first copy only %d" % (int(on.sum()), int(tie.sum()), int(first.sum())))
    assert tie.sum() >= len(r) // 4
    assert (rows[on, MAT] != cc.DUP_FLOOR).all()
    # a tie is one: the flat list without the later copies puts the first copy at the same t
    import oracle
    from rtamd import scene as g
    s = cc.scene("dup")
    only = g.make_scene([s.obj_list[0], g.make_bvh_node([s.obj_list[1].args[0][0]], 0, 0)], s.camera, s.sky_function)
    with np.errstate(all="ignore"):
        alone = oracle.build_scene(only).step(r.rays, 1, sc.SEED, sc.SMP)[0]
    assert sc.same_bits(alone[tie, T], rows[tie, T]).all() and (alone[tie, MAT] == cc.DUP_FIRST).all()


def test_flat_class_hits_flat_curves(oracle_mod):
    """`flat`: at least a quarter of the records end on a flat curve (a curve hit with the flat curves' material;
    the polyline curves are red)."""
    r = cc.records(oracle_mod, "curve_mix_flat")["flat"]
    rows = _rows(oracle_mod, "curve_mix_flat", r)
    flat = cc.curve_hit(rows, r.rays) & (rows[:, MAT] == cc.MIX_WHITE)
    print("flat: %d of %d records hit a flat curve" % (int(flat.sum()), len(r)))
    assert flat.sum() >= len(r) // 4


def test_moving_class_meets_spheres_where_they_are(oracle_mod):
    """`moving`: every shutter time occurs, and the closest hit is a sphere at some and a curve at others."""
    r = cc.records(oracle_mod, "curve_mix")["moving"]
    assert set(r.rays[:, 6]) == {0.0, 0.5, 1.0}
    rows = _rows(oracle_mod, "curve_mix", r, 0)
    on = cc.curve_hit(rows, r.rays)
    sphere = (rows[:, HIT] == 1) & ~on & (np.abs(rows[:, 21:24]).max(axis=1) < 1.0)      # not an axis normal
    assert sphere.sum() >= 32 and on.sum() >= 64, (int(sphere.sum()), int(on.sum()))
    # the time matters: at time 0 some of these records hit something else
    r0 = r.rays.copy()
    r0[:, 6] = 0.0
    with np.errstate(all="ignore"):
        rows0 = cc.oracle_scene(oracle_mod, "curve_mix").step(r0, 0, sc.SEED, sc.SMP)[0]
    assert (~sc.same_bits(rows0[:, T], rows[:, T]) & (r.rays[:, 6] != 0)).sum() >= 16


@pytest.mark.parametrize("name", ["cornell_bezier", "bezier_inst"])
def test_group_curve_records(oracle_mod, name):
    """One curve in a brute-force group, plain and under an instance chain.  A single curve has no neighbour that
    takes the rays its ends and its ribbon's edge let through, so `ends` holds fewer hits than in the curve
    clouds (a seventh: by its construction half the records pass outside the edge, and at u = 0 and 1 the
    parameter's end lets half of the rest by); `leave` starts on the curve and mostly leaves it."""
    recs = cc.records(oracle_mod, name)
    for cls, least in (("vertical", 4), ("ends", 10)):
        r = recs[cls]
        rows = _rows(oracle_mod, name, r)
        on = cc.curve_hit(rows, r.rays) if name == "cornell_bezier" else \
            (rows[:, HIT] == 1) & (rows[:, MAT] == cc.INST_CURVE_MAT)
        print("%-14s %-9s records %d: curve hits %d" % (name, cls, len(r), int(on.sum())))
        assert on.sum() * least >= len(r) and (~on).sum() * 10 >= len(r), (name, cls, int(on.sum()))
    assert len(recs["leave"]) >= cc.N // 2 and (recs["leave"].ctr > 0).all()
    if name == "bezier_inst":
        # under the rotation the world normal is no longer -d bit for bit on the oblique rays: the chain is at work
        r = recs["ends"]
        rows = _rows(oracle_mod, name, r)
        on = (rows[:, HIT] == 1) & (rows[:, MAT] == cc.INST_CURVE_MAT)
        assert (~sc.same_bits(rows[on, 21:24], -r.rays[on, 3:6]).all(axis=1)).any()
        assert np.allclose(rows[on, 21:24], -r.rays[on, 3:6], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(cc.KLEIN_MAT))
def test_klein_records(oracle_mod, name):
    recs = cc.records(oracle_mod, name)
    r = recs["klein"]
    rows = _rows(oracle_mod, name, r)
    on = (rows[:, HIT] == 1) & (rows[:, MAT] == cc.KLEIN_MAT[name])
    assert len(r) == cc.N and on.sum() >= len(r) // 2 and (~on).sum() * 10 >= len(r)
    left = recs["klein_leave"]
    assert len(left) >= cc.N // 2 and (left.ctr > 0).all()


@pytest.mark.parametrize("name", list(cc.CASES) + list(cc.GROUP_CASES))
def test_records_are_finite_and_directed(oracle_mod, name):
    """No non-finite component and no zero direction goes to a curve scene (Recs asserts it where it is built)."""
    for cls, r in cc.records(oracle_mod, name).items():
        assert np.isfinite(r.rays).all() and (np.abs(r.rays[:, 3:6]).max(axis=1) > 0).all(), (name, cls)
        assert ((r.rays[:, 6] == 0) | (cls == "moving")).all()


@pytest.mark.parametrize("name", ["curves_small", "curve_mix", "dup", "cornell_bezier", "bezier_inst", "cornell_klein"])
def test_step_iterated_equals_color_from(oracle_mod, name):
    """orc_step iterated to the end of every path is orc_color_from, on every third record of the new classes."""
    osc = cc.oracle_scene(oracle_mod, name)
    new = cc.CASES[name][2] if name in cc.CASES else cc.GROUP_CASES[name][1]
    for cls in new:
        r = cc.records(oracle_mod, name)[cls]
        depth = 0 if cls == "moving" else 1
        rays, ctr = r.rays[::3], r.ctr[::3]
        with np.errstate(all="ignore"):
            want = osc.color_from(rays, depth, sc.SEED, sc.SMP, ctr_in=ctr)
        got = sc.iterate_oracle(osc, rays, depth, ctr=ctr)
        assert sc.same_bits(got, want).all(), (name, cls)
