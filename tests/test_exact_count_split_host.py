"""The split counting search without a GPU: its Python statement (tests/exact_count_split_model.py) against the plain counting search's
(tests/exact_count_model.py) at every depth, the leaf inside the prefix, the counts that round, the per-cube budget, the header and the
refusals of count_models(split=...)."""
import functools
import os
import re

import numpy as np
import pytest

import exact_count_cases as cs
import exact_count_model as cm
import exact_count_split_model as sm
from helpers import REPO


@functools.lru_cache(maxsize=None)
def instances():
    return cs.family() + [cs.fan(k) for k in cs.FAN_K]


@functools.lru_cache(maxsize=None)
def plain():
    return [cm.search(n, c) for n, c in instances()]


def test_depth_zero_is_the_plain_search():
    inst = instances()
    assert len(inst) >= 400
    for (n, c), want in zip(inst, plain()):
        st, count, tc, work, leaves, cubes = sm.search(n, c, depth=0)
        assert (st, count, work, leaves) == (want[0], want[1], want[3], want[4])
        assert tc.dtype == np.float64
        np.testing.assert_array_equal(tc, want[2])
        assert cubes == [(st, count, work, leaves)]


@pytest.mark.parametrize('depth', [1, 2, 3, 4, 5, 6])
def test_cubes_add_up_to_the_plain_count(depth):
    # the fans round (count 2^k + 1): their sum is pinned to the model's own order below, everything else is exact and equal
    inst, want = instances(), plain()
    replayed = 0
    for (n, c), w in zip(inst, want):
        if w[1] > 2.0 ** 53:
            continue
        st, count, tc, work, leaves, cubes = sm.search(n, c, depth=depth)
        assert (st, count, leaves) == (w[0], w[1], w[4])
        np.testing.assert_array_equal(tc, w[2])
        assert len(cubes) == 1 << depth
        assert sum(cb[3] for cb in cubes) == w[4] and sum(cb[2] for cb in cubes) == work
        assert all(cb[1] == float(int(cb[1])) for cb in cubes)
        e = sum(len(x) for x in c)
        assert w[3] <= work < len(cubes) * ((1 << 32) + 3 * e)
        replayed += work > w[3]
    assert replayed > 100


def test_a_leaf_inside_the_prefix_goes_to_one_cube():
    # n = 3 cannot open eight levels: every leaf lies inside the prefix
    n, clauses = 3, [[1, 2], [-1, 3]]
    want = cm.search(n, clauses)
    st, count, tc, work, leaves, cubes = sm.search(n, clauses, depth=8)
    assert (st, count, leaves) == (1, want[1], want[4]) and count == 4.0
    np.testing.assert_array_equal(tc, want[2])
    credited = [j for j, cb in enumerate(cubes) if cb[3] > 0]
    assert len(credited) == want[4] and sum(cubes[j][1] for j in credited) == 4.0
    # a leaf was met with L <= 3 levels open by the 2^(8-L) cubes that share its top L bits: the one credited has its other bits 0, and
    # each of the others made the same reads for nothing
    for j in credited:
        assert j & 31 == 0
        assert all(cubes[i][1:] == (0.0, cubes[j][2], 0) for i in range(j + 1, j + 32))
    # the first propagation alone satisfies everything: the leaf has no level open, and cube 0 alone is credited
    n, clauses = 5, [[1], [-1, 2], [-2, 3]]
    for depth in (1, 4):
        st, count, tc, work, leaves, cubes = sm.search(n, clauses, depth=depth)
        assert (st, count, leaves) == (1, 4.0, 1)
        assert cubes[0][1:] == (4.0, cubes[0][2], 1) and all(cb[1] == 0.0 and cb[3] == 0 for cb in cubes[1:])
        assert len({cb[2] for cb in cubes}) == 1                                      # every cube made the same reads
        np.testing.assert_array_equal(tc, cm.search(n, clauses)[2])


def test_fans_round_in_the_split_order():
    for k in cs.FAN_K:
        n, clauses = cs.fan(k)
        st, count, tc, work, leaves, cubes = sm.search(n, clauses, depth=2)
        assert st == 1 and leaves == 2 and len(cubes) == 4
        total, tsum = 0.0, np.zeros(n)
        for j in range(4):
            r = sm.cube(n, clauses, 0, 2, j)
            total = total + r[1]
            tsum = tsum + r[2]
        assert count == total and count >= 2.0 ** k
        np.testing.assert_array_equal(tc, tsum)
        assert abs(count - cm.search(n, clauses)[1]) <= 2.0 ** (k - 52)


def test_budget_is_per_cube():
    inst = cs.family()[::6] + cs.uniform_3sat(3, 20, (3.5, 4.0), 4)
    full = [cm.search(n, c) for n, c in inst]
    seen = set()
    for budget in (50, 500, 5000):
        for depth in (1, 3):
            for (n, c), f in zip(inst, full):
                st, count, tc, work, leaves, cubes = sm.search(n, c, budget, depth)
                e = sum(len(x) for x in c)
                assert st == (-1 if any(cb[0] == -1 for cb in cubes) else 1)
                assert count <= f[1] and leaves <= f[4] and (tc <= f[2]).all()
                for cb in cubes:
                    assert cb[2] < budget + 3 * e and (cb[0] == 1 or cb[2] >= budget)
                assert work < len(cubes) * (budget + 3 * e)
                if st == 1:
                    assert count == f[1] and leaves == f[4]
                    np.testing.assert_array_equal(tc, f[2])
                seen.add(st)
    assert seen == {-1, 1}


def test_too_many_variables_at_every_depth():
    for depth in (0, 1, 7, 16):
        st, count, tc, work, leaves, cubes = sm.search(1024, [[1, 2], [-1, 1024]], depth=depth)
        assert (st, count, work, leaves) == (-2, 0.0, 0, 0) and tc.shape == (1024,) and not tc.any()
        assert cubes == [(-2, 0.0, 0, 0)]


def test_header_and_symbols():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    assert '#define PDP_ABI_VERSION 3' in text
    assert ("int pdp_exact_count_split(pdp_problem *p, const int8_t *depth, int64_t budget, int8_t *status, double *count, double *true_count, "
            "int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream);") in text
    assert ("int pdp_exact_count_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, double *cube_count, int64_t *cube_work, "
            "int64_t *cube_leaves, void *stream);") in text
    from pdp import native
    assert {'pdp_exact_count_split', 'pdp_exact_count_split_cubes'} <= set(native.EXPORTED_SYMBOLS)


@pytest.mark.parametrize('split', [17, -1, True, 'x'])
def test_count_models_refuses_a_bad_split(split):
    from pdp import exact
    with pytest.raises(ValueError, match='split must be'):
        exact.count_models([exact.raw_item(2, [[1, 2]])], split=split)
