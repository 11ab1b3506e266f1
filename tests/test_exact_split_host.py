"""The split complete search stated in Python (tests/exact_split_model.py, pdp_exact_solve_split): depth 0 is exact_model.search, the lowest
satisfiable cube carries the plain search's model at every depth, the budget applies per cube, and the host entry points refuse what the
split does not cover.  No GPU."""
import os
import re

import numpy as np
import pytest

import exact_count_cases as cs
import exact_model as em
import exact_split_model as sm
from helpers import REPO


def hint_sets(rng, n, clauses):
    "no hints, random complete hints, hints with NaN among them, and (where the instance has a model) that model as complete hints"
    out = [None, rng.rand(n).astype(np.float32)]
    h = rng.rand(n).astype(np.float32)
    h[rng.rand(n) < 0.4] = np.nan
    out.append(h)
    st, model, _ = em.search(n, clauses)
    if st == 1:
        out.append(model.copy())
    return out


def width(n, clauses):
    return max([n] + [abs(int(l)) for c in clauses for l in c])


def test_depth_zero_is_the_plain_search():
    rng = np.random.RandomState(901)
    accepted = rejected = 0
    for n, clauses in cs.family():
        for hints in hint_sets(rng, width(n, clauses), clauses):
            for budget in (em.NO_BUDGET, 40):
                want = em.search(n, clauses, hints, budget)
                got = sm.search(n, clauses, hints, budget, 0)
                assert got[0] == want[0] and got[2] == want[2] and np.array_equal(got[1], want[1]) and got[1].dtype == np.float32
                accepted += got[3] == -1 and got[0] == 1 and not got[4]
                rejected += len(got[4]) == 1
    assert accepted > 100 and rejected > 1000


def test_every_depth_gives_the_plain_status_and_model():
    rng = np.random.RandomState(902)
    sat = unsat = late = 0
    for n, clauses in cs.family():
        hints = hint_sets(rng, width(n, clauses), clauses)[int(rng.randint(3))]
        want = em.search(n, clauses, hints)
        for depth in range(1, 7):
            st, model, work, first, cubes = sm.search(n, clauses, hints, depth=depth)
            assert st == want[0] and np.array_equal(model, want[1])
            if st == 1 and cubes:
                assert first == len(cubes) - 1 and cubes[-1][0] == 1 and all(c[0] == 0 for c in cubes[:-1])
                late += first > 0
            else:
                assert first == -1 and (not cubes or (len(cubes) == 1 << depth and all(c[0] == 0 for c in cubes)))
            assert work >= sum(c[1] for c in cubes)
        sat += want[0] == 1
        unsat += want[0] == 0
    assert sat > 100 and unsat > 50 and late > 50            # late: (instance, depth) pairs whose model lies past cube 0


def test_budget_per_cube():
    inst = cs.family()[::7] + cs.uniform_3sat(903, 24, (4.0, 4.6), 6)
    seen = set()
    passed_over = 0
    for n, clauses in inst:
        e = sum(len(c) for c in clauses)
        full = em.search(n, clauses)
        for budget in (50, 500, 5000):
            for depth in (0, 2, 4):
                st, model, work, first, cubes = sm.search(n, clauses, None, budget, depth)
                assert all(w < budget + 3 * max(e, 1) for _, w in cubes) and all(w >= budget for s, w in cubes if s == -1)
                assert work == sum(w for _, w in cubes) and work < max(1, len(cubes)) * (budget + 3 * max(e, 1))
                if st == 1:
                    assert first == len(cubes) - 1 and full[0] == 1 and em.check_reads(clauses, model)[1]
                    if any(s == -1 for s, _ in cubes[:-1]):
                        passed_over += 1                     # a model from a later cube than the plain search's first
                    else:
                        assert np.array_equal(model, full[1])
                elif st == 0:
                    assert full[0] == 0 and all(s == 0 for s, _ in cubes) and len(cubes) == 1 << depth
                else:
                    assert any(s == -1 for s, _ in cubes) and not any(s == 1 for s, _ in cubes) and not model.any()
                seen.add((int(st), depth > 0))
    assert seen == {(s, d) for s in (1, 0, -1) for d in (False, True)}
    assert passed_over > 0                                   # status 1 although a lower cube ran out of budget


def test_check_reads_count_against_every_cube():
    "a rejected check pass: its reads are on every cube's counter, as they are on the plain search's"
    n, clauses = cs.uniform_3sat(904, 20, (4.26,), 1)[0]
    hints = np.zeros(n, dtype=np.float32)
    reads, ok = em.check_reads(clauses, hints)
    assert not ok
    st, _, w = sm.cube(n, clauses, hints, reads + 1, 2, 0, spent=reads)
    assert (st, w > 0) == (-1, True) and reads + w < reads + 1 + 3 * sum(len(c) for c in clauses)
    assert sm.cube(n, clauses, hints, reads, 2, 0, spent=reads)[2] == 0
    got = sm.search(n, clauses, hints, reads, 2)
    assert got[0] == -1 and got[2] == reads and got[4] == [(-1, 0)] * 4


def test_depth_beyond_the_variables():
    inst = [(3, [[1, 2, 3], [-1, -2], [-2, -3], [2, 3]]), (3, [[1, 2], [-1, 2], [1, -2], [-1, -2], [3, 1]]), (3, [[1, 2, 3]])]
    for n, clauses in inst:
        want = em.search(n, clauses)
        st, model, work, first, cubes = sm.search(n, clauses, depth=8)
        assert st == want[0] and np.array_equal(model, want[1])
        assert len(cubes) == (first + 1 if st == 1 else 256)
        # the bits of levels that never open change nothing: cubes that share the bits of the levels that exist are one search
        assert sm.cube(n, clauses, None, 0, 8, 0)[::2] == sm.cube(n, clauses, None, 0, 8, 1)[::2]


def test_degenerate_instances():
    for n, clauses in cs.DEGENERATE:
        want = em.search(n, clauses)
        for depth in (0, 1, 3):
            st, model, work, first, cubes = sm.search(n, clauses, depth=depth)
            assert st == want[0] and np.array_equal(model, want[1])
            assert first == (0 if st == 1 else -1)          # nothing here branches before its first answer
            if depth == 0:
                assert work == want[2]


def test_header_carries_both_prototypes():
    text = open(os.path.join(REPO, 'include', 'pdp_hip.h')).read()
    flat = re.sub(r'\s+', ' ', text)
    assert ('int pdp_exact_solve_split(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, float *model, '
            'int64_t *work, int32_t *first, int8_t *depth_used, void *stream);') in flat
    assert 'int pdp_exact_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int64_t *cube_work, void *stream);' in flat
    assert '#define PDP_ABI_VERSION 3' in text
    from pdp import native
    assert {'pdp_exact_solve_split', 'pdp_exact_split_cubes'} <= set(native.EXPORTED_SYMBOLS)


def test_solve_items_refuses_split_with_the_other_searches():
    from pdp import exact
    items = [exact.raw_item(3, [[1, 2], [-1, 3]])]
    for more in (dict(learn=True), dict(certify=True), dict(assume=[np.array([1, 0, 0])])):
        for split in (4, 'auto'):
            with pytest.raises(ValueError, match='split spreads the plain search'):
                exact.solve_items(items, split=split, **more)
    for wrong in (-1, 17, 2.0, True, 'deep'):
        with pytest.raises(ValueError, match='split must be'):
            exact.solve_items(items, split=wrong)
    with pytest.raises(ValueError, match='split spreads the plain search'):
        exact.is_sat(3, [[1, 2]], learn=True, split=2)
