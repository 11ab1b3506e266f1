"""The split weighted counting search without a GPU: its Python statement (tests/exact_mass_split_model.py) against exact rational
arithmetic at every depth, against the plain statement (tests/exact_mass_model.py) at depth 0, against the split count's statement at
weights 0.5, the two ownership rules (a leaf and the budget's node inside the prefix), 0/1 weights, the per-cube budget's bracket, the
refused instances, the header, the refusals of solution_mass(split=...) and the logit gradient."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import exact_count_cases as cs
import exact_count_split_model as sm
import exact_mass_cases as zc
import exact_mass_model as zm
import exact_mass_split_model as zs
import exact_model
from helpers import REPO

DEPTHS = (0, 1, 2, 3, 4, 5, 6)


@functools.lru_cache(maxsize=None)
def eighths():
    "exact_count_cases.family() (n <= 12) with weights that are multiples of 1/8: [(n, clauses, weights, Z, true, plain result)]"
    out = []
    for (n, c), w in zip(cs.family(), zc.family_weights('eighths')):
        n = zc.size((n, c))
        z, true = zc.brute(n, c, w)
        out.append((n, c, w, z, true, zm.search(n, c, w)))
    return out


@pytest.mark.parametrize('depth', DEPTHS)
def test_cubes_add_up_to_the_rational_mass(depth):
    # a product of at most 12 multiples of 1/8 has at most 36 mantissa bits and a sum of such terms at most 36 + 12: every operation is
    # exact, so the split sums equal the rational values, and the plain search's, bit for bit
    cases = eighths()
    assert len(cases) >= 400 and max(k[0] for k in cases) <= 12
    replayed = 0
    for n, c, w, z, true, plain in cases:
        st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, c, w, depth=depth)
        assert (st, open_mass, used, len(cubes)) == (1, 0.0, depth, 1 << depth)
        assert tm.dtype == np.float64 and tm.shape == (n,)
        assert Fraction(mass) == z and [Fraction(float(x)) for x in tm] == true
        assert leaves == plain[5] and sum(cb[4] for cb in cubes) == leaves and sum(cb[3] for cb in cubes) == work
        assert all(cb[0] == 1 and cb[2] == 0.0 for cb in cubes)
        e = sum(len(x) for x in c)
        assert plain[4] <= work < len(cubes) * ((1 << 32) + 3 * e)
        replayed += work > plain[4]
    assert depth == 0 or replayed > 100


def test_depth_zero_is_the_plain_search():
    inst = cs.family() + [cs.fan(k) for k in cs.FAN_K]
    for kind in ('eighths', 'random', 'half'):
        rng = np.random.RandomState(5)
        weights = zc.family_weights(kind) + [rng.rand(zc.size(cs.fan(k))).astype(np.float32) for k in cs.FAN_K]
        for budget in (0, 60):
            for (n, c), w in zip(inst[::3], weights[::3]):
                want = zm.search(n, c, w, budget)
                got = zs.search(n, c, w, budget, 0)
                assert got[:2] == want[:2] and got[3:6] == want[3:6] and got[6] == 0
                assert got[2].dtype == np.float64
                np.testing.assert_array_equal(got[2], want[2])
                assert got[7] == [(want[0], want[1], want[3], want[4], want[5])]


@pytest.mark.parametrize('depth', [1, 3, 6])
def test_half_weights_are_the_split_count_record_for_record(depth):
    inst = cs.family()[::2] + [cs.fan(k) for k in cs.FAN_K]
    for budget in (0, 60):
        for n, c in inst:
            n = zc.size((n, c))
            if n > 60 and depth > 2:
                continue                                                                  # the fans: three chunks on one level, once is enough
            cst, count, tc, cwork, cleaves, ccubes = sm.search(n, c, budget, depth)
            st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, c, zc.half(n), budget, depth)
            assert (st, work, leaves) == (cst, cwork, cleaves)
            assert len(cubes) == len(ccubes)
            for cb, cc in zip(cubes, ccubes):
                assert (cb[0], cb[3], cb[4]) == (cc[0], cc[2], cc[3]) and cb[1] * 2.0 ** n == cc[1]
            if count <= 2.0 ** 53:
                assert mass * 2.0 ** n == count and np.array_equal(tm * 2.0 ** n, tc)


def test_random_weights_within_the_derived_bound():
    # per cube the error is the plain search's bound on the cube's own share; the sum over cubes adds one rounding per cube on a value
    # of at most Z*: (n + 6 + leaves + cubes) u Z*, and likewise for true_mass -- the bounds of exact_mass_model with leaves + cubes
    inst = zc.small()[0]
    for depth in (1, 4):
        for (n, c), w in list(zip(inst, zc.small_random()))[::2]:
            n = zc.size((n, c))
            z, true = zc.brute(n, c, w)
            st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, c, w, depth=depth)
            assert st == 1 and open_mass == 0.0
            k = leaves + len(cubes)
            assert abs(Fraction(mass) - z) <= Fraction(zm.mass_bound(n, k, 1.0)) * z, (n, c, w.tolist())
            assert max(abs(Fraction(float(x)) - t) for x, t in zip(tm, true)) <= Fraction(zm.true_mass_bound(n, k, 1.0)) * z
            assert leaves == zm.search(n, c, w)[5]


def test_a_leaf_inside_the_prefix_goes_to_one_cube():
    # n = 3 cannot open eight levels: every leaf lies inside the prefix
    n, clauses = 3, [[1, 2], [-1, 3]]
    w = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    want = zm.search(n, clauses, w)
    st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, clauses, w, depth=8)
    assert (st, mass, open_mass, leaves) == (1, want[1], 0.0, want[5]) and Fraction(mass) == zc.brute(n, clauses, w)[0]
    np.testing.assert_array_equal(tm, want[2])
    credited = [j for j, cb in enumerate(cubes) if cb[4] > 0]
    assert len(credited) == want[5] and sum(cubes[j][1] for j in credited) == mass
    for j in credited:
        assert j & 31 == 0
        assert all(cubes[i][1:] == (0.0, 0.0, cubes[j][3], 0) for i in range(j + 1, j + 32))
    # the first propagation alone satisfies everything: the leaf has no level open, and cube 0 alone is credited
    n, clauses = 5, [[1], [-1, 2], [-2, 3]]
    w = np.array([0.5, 0.25, 0.75, 0.125, 1.0], dtype=np.float32)
    for depth in (1, 4):
        st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, clauses, w, depth=depth)
        assert (st, mass, leaves) == (1, 0.5 * 0.25 * 0.75, 1)
        assert cubes[0][1:] == (mass, 0.0, cubes[0][3], 1) and all(cb[1] == 0.0 and cb[4] == 0 for cb in cubes[1:])
        assert len({cb[3] for cb in cubes}) == 1                                          # every cube made the same reads
        np.testing.assert_array_equal(tm, zm.search(n, clauses, w)[2])


def test_the_node_the_budget_fires_at_goes_to_one_cube():
    # a budget of one read per cube at depth 6 on 3-SAT: the first pass meets no unit, so every cube runs out behind its first (pinned)
    # decision.  The 32 cubes of either half stand at the same node, which the one with the low five bits 0 owns: without the ownership
    # rule the open masses would add up to 32
    for (n, c), model in zc.satisfiable_3sat(632, 20, (3.0, 4.0), 2):
        cubes = zs.search(n, c, zc.around(model, 0.75), 1, 6)[7]
        assert all(cb[0] == -1 and cb[1] == 0.0 and cb[4] == 0 for cb in cubes) and len({cb[3] for cb in cubes}) == 1
        assert [cb[2] for cb in cubes] == [0.75] + [0.0] * 31 + [0.25] + [0.0] * 31
    seen_below_one = 0
    for (n, c), w in list(zip(cs.family(), zc.family_weights('eighths')))[::4] + list(zip(cs.family(), zc.family_weights('random')))[1::4]:
        n = zc.size((n, c))
        for budget in (1, 20, 60):
            st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, c, w, budget, 6)
            total = Fraction(mass) + Fraction(open_mass)
            if all(float(x) * 8 == int(float(x) * 8) for x in w):
                assert total <= 1, (n, c, w.tolist(), budget)
            else:
                assert total <= 1 + Fraction(zm.mass_bound(n, leaves + 64, 1.0))
            seen_below_one += total < 1
    assert seen_below_one > 0


def test_zero_one_weights():
    inst = [i for i in cs.family() if zc.size(i) > 0][::3] + [i for i, _ in zc.satisfiable_3sat(17, 20, (3.5, 4.0), 2)]
    sat = 0
    for n, c in inst:
        n = zc.size((n, c))
        st, model, _ = exact_model.search(n, c)
        if st != 1:
            continue
        sat += 1
        w = np.asarray(model, dtype=np.float32)
        for depth in (1, 3, 6):
            zst, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, c, w, depth=depth)
            assert (zst, mass, open_mass, leaves) == (1, 1.0, 0.0, 1) and np.array_equal(tm, w.astype(np.float64))
            assert sum(cb[1] for cb in cubes) == 1.0 and sum(1 for cb in cubes if cb[1] > 0) == 1
        clause = next((k for k in c if k and not any(-l in k for l in k)), None)
        if clause is not None:
            w = w.copy()
            for l in clause:                                                              # every literal of one clause false: not a model
                w[abs(l) - 1] = 0.0 if l > 0 else 1.0
            zst, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, c, w, depth=3)
            assert (zst, mass, open_mass, leaves) == (1, 0.0, 0.0, 0) and not tm.any()
    assert sat >= 100


def test_budget_is_per_cube_and_brackets_the_mass():
    cases = zc.satisfiable_3sat(631, 24, (3.0, 4.0), 2)
    inst = [(i, zc.around(m, conf)) for i, m in cases for conf in (0.5, 0.75, 0.9)]
    inst += [(i, w) for i, w in list(zip(cs.family(), zc.family_weights('eighths')))[::12]]
    seen = set()
    for (n, c), w in inst:
        n = zc.size((n, c))
        full = zm.search(n, c, w)
        assert full[0] == 1
        e = sum(len(x) for x in c)
        for budget in (20, 200, 2000):
            for depth in (1, 3):
                got = zs.search(n, c, w, budget, depth)
                st, mass, tm, open_mass, work, leaves, used, cubes = got
                assert st == (-1 if any(cb[0] == -1 for cb in cubes) else 1)
                for cb in cubes:
                    assert cb[3] < budget + 3 * e and (cb[0] == 1 or cb[3] >= budget) and (cb[0] == -1 or cb[2] == 0.0)
                assert work < len(cubes) * (budget + 3 * e) and leaves <= full[5]
                # mass <= Z <= mass + open_mass <= 1, up to the rounding of the sums
                k = full[5] + len(cubes)
                slack = Fraction(zm.mass_bound(n, k, 1.0))
                assert Fraction(mass) <= Fraction(full[1]) * (1 + slack)
                assert Fraction(full[1]) <= (Fraction(mass) + Fraction(open_mass)) * (1 + slack) + slack * Fraction(full[1])
                assert Fraction(mass) + Fraction(open_mass) <= 1 + slack
                assert (tm <= full[2] * (1 + float(zm.true_mass_bound(n, k, 1.0))) + zm.true_mass_bound(n, k, full[1])).all()
                if st == 1:
                    assert open_mass == 0.0 and leaves == full[5]
                    assert abs(mass - full[1]) <= zm.mass_bound(n, k, full[1])
                seen.add(st)
    assert seen == {-1, 1}


def test_refused_instances_at_every_depth():
    for depth in (0, 1, 7, 16):
        n = 1024
        st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(n, [[1, 2], [-1, 1024]], zc.half(n), depth=depth)
        assert (st, mass, open_mass, work, leaves, used) == (-2, 0.0, 0.0, 0, 0, 0) and tm.shape == (n,) and not tm.any()
        assert cubes == [(-2, 0.0, 0.0, 0, 0)]
    for depth in (0, 1, 5):
        for bad in (np.nan, 1.5, -0.1):
            w = np.array([0.25, bad, 0.75], dtype=np.float32)
            st, mass, tm, open_mass, work, leaves, used, cubes = zs.search(3, [[1, 2], [-2, 3]], w, depth=depth)
            assert (st, mass, open_mass, work, leaves, used) == (-3, 0.0, 0.0, 0, 0, depth) and tm.shape == (3,) and not tm.any()
            assert cubes == [(-3, 0.0, 0.0, 0, 0)] * (1 << depth)


def test_header_and_symbols():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    assert '#define PDP_ABI_VERSION 3' in text
    assert ("int pdp_exact_mass_split(pdp_problem *p, const float *weights, const int8_t *depth, int64_t budget, int8_t *status, double *mass, "
            "double *true_mass, double *open_mass, int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream);") in text
    assert ("int pdp_exact_mass_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, double *cube_mass, double *cube_open, "
            "int64_t *cube_work, int64_t *cube_leaves, void *stream);") in text
    from pdp import native
    assert {'pdp_exact_mass_split', 'pdp_exact_mass_split_cubes'} <= set(native.EXPORTED_SYMBOLS)
    assert hasattr(native.lib(), 'pdp_exact_mass_split') and hasattr(native.lib(), 'pdp_exact_mass_split_cubes')


@pytest.mark.parametrize('split', [17, -1, True, 'x'])
def test_solution_mass_refuses_a_bad_split(split):
    from pdp import exact
    with pytest.raises(ValueError, match='split must be'):
        exact.solution_mass([exact.raw_item(2, [[1, 2]])], [np.array([0.5, 0.5], dtype=np.float32)], split=split)


def test_the_logit_gradient_is_the_derivative_of_the_loss():
    # d(-ln Z)/d logit_v = -p_v (1 - p_v) (Z1 - Z0) / Z with Z1 / Z0 the masses under v true / false, from brute force in Fractions;
    # mass_logit_gradient forms it as p_v - posterior_v
    from pdp import exact
    inst, weights = zc.small()
    checked = 0
    for (n, c), w, (z, true) in list(zip(inst, weights, zc.small_brute()))[::5]:
        n = zc.size((n, c))
        if z == 0:
            assert not exact.mass_logit_gradient([w], [None])[0].any()
            continue
        posterior = np.array([float(t / z) for t in true], dtype=np.float64)
        got = exact.mass_logit_gradient([w], [posterior])[0]
        assert got.dtype == np.float64 and got.shape == (n,)
        for v in range(n):
            p = Fraction(float(w[v]))
            one, zero = w.copy(), w.copy()
            one[v], zero[v] = 1.0, 0.0
            z1, z0 = zc.brute(n, c, one)[0], zc.brute(n, c, zero)[0]
            assert z == p * z1 + (1 - p) * z0                                             # Z is multilinear
            want = -p * (1 - p) * (z1 - z0) / z
            assert abs(Fraction(float(got[v])) - want) <= Fraction(2.0 ** -52)
        checked += 1
    assert checked >= 10
    with pytest.raises(ValueError, match='one array per instance'):
        exact.mass_logit_gradient([np.zeros(2)], [])
    with pytest.raises(ValueError, match='must have 2 values'):
        exact.mass_logit_gradient([np.zeros(2)], [np.zeros(3)])
