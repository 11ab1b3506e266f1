"""The split optimising search without a GPU: its Python statement (tests/exact_min_unsat_split_model.py) against the plain search's
(tests/exact_min_unsat_model.py) -- depth 0 equal in all five outputs under every budget, the optimum at depths 1..6 under the sequential
and under randomly interleaved schedules of the cubes, brute force, a leaf inside the prefix, an optimal hint, a satisfiable instance, the
per-cube budget -- and the header and the refusals of exact.min_unsat(split=...)."""
import os
import re

import numpy as np
import pytest

import exact_min_unsat_model as mm
import exact_min_unsat_split_cases as sc
import exact_min_unsat_split_model as sm
from helpers import REPO


def attains(clauses, res):
    "the model of a result leaves exactly its cost unsatisfied, and the cube that holds it says so"
    status, cost, model, work, improvements, first, cubes = res
    assert model.dtype == np.float32 and mm.unsat_count(clauses, model) == cost
    assert first == -1 or cubes[first][2] == cost
    assert all(c[2] == sm.NO_COST or c[2] >= cost for c in cubes)
    assert improvements == sum(c[3] for c in cubes) and (first >= 0) == any(c[2] == cost for c in cubes)


@pytest.mark.parametrize('kind', sc.KINDS)
def test_depth_zero_is_the_plain_search(kind):
    inst, hints = sc.family()
    assert len(inst) >= 120
    for budget in (0, 50, 500, 5000):
        seen = set()
        for (n, c), h in zip(inst, hints[kind]):
            want = mm.search(n, c, h, budget)
            got = sm.sequential(n, c, h, budget, 0)
            assert got[:2] == want[:2] and got[3:5] == want[3:5]
            assert got[2].dtype == want[2].dtype and np.array_equal(got[2], want[2])
            assert len(got[6]) == 1 and got[6][0][0] == want[0] and got[6][0][3] == want[4]
            seen.add(want[0])
        assert seen == {1} if budget == 0 else (seen == {-1, 1} or budget > 50)


@pytest.mark.parametrize('depth', [1, 2, 3, 4, 5, 6])
def test_the_optimum_at_every_depth_and_under_any_schedule(depth):
    inst, hints = sc.family()
    brute = sc.family_brute()
    improved = shared = 0
    for j, (n, c) in enumerate(inst):
        for kind in sc.KINDS:
            h = hints[kind][j]
            want = mm.search(n, c, h)
            assert want[0] == 1 and want[1] == brute[j]
            runs = [sm.sequential(n, c, h, 0, depth)]
            if kind == 'random':
                runs += [sm.interleaved(n, c, h, 0, depth, seed=s, width=w) for s, w in ((0, 8), (1, 3), (2, 64))]
            for res in runs:
                assert res[0] == 1 and res[1] == want[1] and len(res[6]) == 1 << depth
                attains(c, res)
                assert all(st == 1 for st, _, _, _ in res[6])
                assert res[3] == sm.check(n, c, h)[4] + sum(w for _, w, _, _ in res[6])
            improved += runs[0][4] > 0
            shared += sum(1 for cu in runs[0][6] if cu[3] > 0) > 1
    assert improved > 50 and shared > 5              # incumbents were replaced, and by more than one cube of an instance


def test_a_leaf_inside_the_prefix_belongs_to_one_cube():
    n, clauses = sc.prefix_only()
    want = mm.search(n, clauses)
    assert want[:2] == (1, 1) and want[4] >= 1
    res = sm.sequential(n, clauses, None, 0, 8)
    assert res[:2] == (1, 1) and len(res[6]) == 256
    attains(clauses, res)
    # at most 8 assignments exist: a leaf shared by many cubes is credited to one of them, so no more than 8 cubes ever accept one
    assert 1 <= res[4] <= 8 and sum(1 for c in res[6] if c[3] > 0) <= 8
    for s in range(4):
        got = sm.interleaved(n, clauses, None, 0, 8, seed=s, width=32)
        assert got[:2] == (1, 1)
        attains(clauses, got)


def test_an_optimal_hint_stays():
    inst, hints = sc.family()
    met = 0
    for (n, c), h in zip(inst, hints['random']):
        best = mm.search(n, c, h)
        if best[1] == 0 or not len(c):
            continue
        for depth in (0, 3):
            res = sm.sequential(n, c, best[2], 0, depth)
            assert res[:2] == (1, best[1]) and res[4] == 0 and res[5] == -1 and np.array_equal(res[2], best[2])
            assert all(cu[2] == sm.NO_COST for cu in res[6])
        met += 1
    assert met > 20


def test_cost_zero_stops_every_cube():
    inst, hints = sc.family()
    met = 0
    for (n, c), h in zip(inst, hints['random']):
        plain = mm.search(n, c, h)
        if plain[1] != 0 or plain[4] == 0:
            continue
        res = sm.sequential(n, c, h, 0, 4)
        assert res[:2] == (1, 0) and mm.unsat_count(c, res[2]) == 0 and res[4] >= 1
        at = res[5]
        assert at >= 0 and all(cu == (1, 0, sm.NO_COST, 0) for cu in res[6][at + 1:])      # the later cubes load 0 and do not start
        # an accepted satisfying hint: no cube is searched at all
        again = sm.sequential(n, c, res[2], 0, 4)
        assert again[:2] == (1, 0) and again[5] == -1 and again[3] == sm.check(n, c, res[2])[4]
        assert all(cu == (1, 0, sm.NO_COST, 0) for cu in again[6])
        met += 1
    assert met > 10


def test_budget_is_per_cube():
    inst, hints = sc.family()
    more = sc.uniform_3sat(3, 20, 1)
    rng = np.random.RandomState(3)
    cases = list(zip(inst[::6], hints['random'][::6])) + [(i, rng.randint(0, 2, size=i[0]).astype(np.float32)) for i in more]
    seen = set()
    for budget in (50, 500, 5000):
        for (n, c), h in cases:
            edges = sum(len(x) for x in c)
            n2, _, _, _, chk, ub0 = sm.check(n, c, h)
            for depth in (0, 2, 4):
                for res in (sm.sequential(n, c, h, budget, depth), sm.interleaved(n, c, h, budget, depth, seed=budget + depth)):
                    status, cost, model, work, _, _, cubes = res
                    attains(c, res)                                               # also under status -1
                    assert cost <= ub0
                    assert status == (1 if all(cu[0] == 1 for cu in cubes) else -1)
                    assert all(w < budget + 3 * edges for _, w, _, _ in cubes)
                    assert all(chk + w >= budget for st, w, _, _ in cubes if st == -1)
                    assert work == chk + sum(w for _, w, _, _ in cubes) and work < chk + len(cubes) * (budget + 3 * edges)
                    seen.add(status)
    assert seen == {-1, 1}


def test_the_large_cases_finish_on_the_model():
    "the n = 20 instances of the GPU batch: the optimum under the sequential and a random schedule, at the depth the batch gives them"
    inst, hints, depth = sc.batch()
    few = len(sc.family()[0])
    for j in range(few, few + 9, 4):
        n, c = inst[j]
        h = hints['random'][j]
        want = mm.search(n, c, h)
        assert want[0] == 1
        for res in (sm.sequential(n, c, h, 0, int(depth[j])), sm.interleaved(n, c, h, 0, int(depth[j]), seed=j, width=16)):
            assert res[0] == 1 and res[1] == want[1]
            attains(c, res)


def test_header_and_symbols():
    from pdp import native
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    assert '#define PDP_ABI_VERSION 3' in text
    assert ("int pdp_exact_min_unsat_split(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, int32_t *cost, "
            "float *model, int64_t *work, int32_t *improvements, int32_t *first, int8_t *depth_used, void *stream);") in text
    assert ("int pdp_exact_min_unsat_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int32_t *cube_cost, int64_t *cube_work, "
            "int32_t *cube_improvements, void *stream);") in text
    assert {'pdp_exact_min_unsat_split', 'pdp_exact_min_unsat_split_cubes'} <= set(native.EXPORTED_SYMBOLS)
    assert 'exact_min_unsat_split' in native.Problem.exact_last_grid.__doc__


@pytest.mark.parametrize('split', [17, -1, True, 'x', 2.0])
def test_min_unsat_refuses_a_bad_split(split):
    from pdp import exact
    with pytest.raises(ValueError, match='split must be'):
        exact.min_unsat([exact.raw_item(2, [[1, 2]])], split=split)
