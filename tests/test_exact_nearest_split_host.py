"""The split nearest-model search without a GPU: its Python statement (tests/exact_nearest_split_model.py) against the plain search's
(tests/exact_nearest_model.py) and brute force -- depth 0 equal in all five outputs under every budget, status and cost at depths 1..6
under the sequential and under randomly interleaved schedules of the cubes, a leaf inside the prefix, a hint that is a model, penalties
of 0, instances without a model, a penalty out of range, start models, the pinned flip, the per-cube budget, the instances of the GPU
batch -- and the header, the symbols and the refusals of exact.nearest_model(split=...)."""
import functools
import os
import re

import numpy as np
import pytest

import exact_nearest_cases as nc
import exact_nearest_model as nm
import exact_nearest_split_cases as sc
import exact_nearest_split_model as sm
from helpers import REPO

NOTHING = (1, 0, sm.NO_COST, 0)         # the record of a cube that did not start


def dressed(mixed):
    inst, hints, pens = nc.small()
    return inst, hints, pens if mixed else [None] * len(inst)


@pytest.mark.parametrize('mixed', [True, False])
def test_depth_zero_is_the_plain_search(mixed):
    inst, hints, pens = dressed(mixed)
    assert len(inst) == 411
    for budget in (0, 1, 50, 500, 5000):
        seen = set()
        for (n, c), h, p in zip(inst, hints, pens):
            want = nm.search(n, c, h, p, budget)
            got = sm.sequential(n, c, h, p, None, budget, 0)
            assert got[:2] == want[:2] and got[3:5] == want[3:5]
            assert got[2].dtype == want[2].dtype and np.array_equal(got[2], want[2])
            assert len(got[7]) == 1 and got[7][0][3] == want[4] and got[6] == -1
            assert got[5] == (0 if want[4] > 0 else -1)
            seen.add(want[0])
        assert seen == ({0, 1} if budget == 0 else {-1, 1}) or budget > 1


@functools.lru_cache(maxsize=None)
def brute_cost(j, mixed):
    "brute force on instance j of small(): the least distance over its models, None without one"
    inst, hints, pens = dressed(mixed)
    n, c = inst[j]
    nn = max([n] + [abs(int(l)) for x in c for l in x])
    return nc.brute(n, c, nm.threshold(nn, hints[j]), nm.penalty_list(nn, pens[j]))[0]


@pytest.mark.parametrize('depth', [1, 2, 3, 4, 5, 6])
def test_status_and_cost_at_every_depth_and_under_any_schedule(depth):
    improved = shared = 0
    for mixed in (True, False):
        inst, hints, pens = dressed(mixed)
        for j, ((n, c), h, p) in enumerate(zip(inst, hints, pens)):
            want = nm.search(n, c, h, p)
            best = brute_cost(j, mixed)
            runs = [sm.sequential(n, c, h, p, None, 0, depth)]
            runs += [sm.interleaved(n, c, h, p, None, 0, depth, seed=s, width=w) for s, w in ((0, 8), (1, 3), (2, 64))]
            for res in runs:
                assert res[:2] == want[:2] == ((0, -1) if best is None else (1, best)) and len(res[7]) == 1 << depth
                sc.attains((n, c), h, p, res)
                assert all(cu[0] == 1 for cu in res[7])
                assert res[3] == sm.check(n, c, h, p)[4] + sum(cu[1] for cu in res[7])
            improved += runs[0][4] > 0
            shared += sum(1 for cu in runs[0][7] if cu[3] > 0) > 1
    assert improved > 100 and shared > 5             # models were replaced, and by more than one cube of an instance


def test_a_leaf_inside_the_prefix_belongs_to_one_cube():
    n, clauses = sc.prefix_only()
    hint = np.array([0, 0, 0], dtype=np.float32)
    want = nm.search(n, clauses, hint)
    assert want[0] == 1 and want[1] == nc.brute(n, clauses, [0, 0, 0], [1, 1, 1])[0] and want[4] >= 1
    res = sm.sequential(n, clauses, hint, None, None, 0, 8)
    assert res[:2] == want[:2] and len(res[7]) == 256
    sc.attains((n, clauses), hint, None, res)
    # at most 8 assignments exist: a leaf shared by many cubes is credited to one of them, so no more than 8 cubes ever accept one
    assert 1 <= res[4] <= 8 and sum(1 for cu in res[7] if cu[3] > 0) <= 8
    for s in range(4):
        got = sm.interleaved(n, clauses, hint, None, None, 0, 8, seed=s, width=32)
        assert got[:2] == want[:2]
        sc.attains((n, clauses), hint, None, got)


def test_the_first_propagation_satisfies_everything_at_depth_six():
    "unit clauses only: the one leaf has no level open, every one of the 64 cubes reaches it and cube 0 owns it"
    n, clauses = 5, [[1], [-2], [3], [1, 4]]
    hint = np.array([0, 0, 0, 1, 1], dtype=np.float32)
    res = sm.sequential(n, clauses, hint, [3, 1, 2, 9, 9], None, 0, 6)
    assert res[:2] == (1, 5) and res[5] == 0 and res[4] == 1 and res[2].tolist() == [1, 0, 1, 1, 1]
    assert res[7][0][2:] == (5, 1) and all(cu[2:] == (sm.NO_COST, 0) and cu[0] == 1 for cu in res[7][1:])
    for s in range(3):
        got = sm.interleaved(n, clauses, hint, [3, 1, 2, 9, 9], None, 0, 6, seed=s, width=64)
        assert got[:2] == (1, 5) and got[5] == 0 and got[4] == 1 and np.array_equal(got[2], res[2])


def test_a_hint_that_is_a_model_starts_no_cube():
    inst, hints, pens = nc.small()
    met = 0
    for (n, c), p in zip(inst, pens):
        m = nc.any_model(n, c)
        if m is None:
            continue
        for depth in (0, 3):
            res = sm.sequential(n, c, m, p, None, 0, depth)
            assert res[:2] == (1, 0) and res[4] == 0 and res[5] == -1 and np.array_equal(res[2], m)
            assert res[3] == sm.check(n, c, m, p)[4] and all(cu == NOTHING for cu in res[7])
        met += 1
    assert met > 100


def test_penalties_of_zero_end_every_cube_at_the_first_accepted_leaf():
    inst, hints, _ = nc.small()
    met = 0
    for (n, c), h in zip(inst, hints):
        nn = max([n] + [abs(int(l)) for x in c for l in x])
        zero = [0] * nn
        plain = nm.search(n, c, h, zero)
        if plain[0] != 1 or plain[4] == 0:
            continue
        res = sm.sequential(n, c, h, zero, None, 0, 4)
        assert res[:2] == (1, 0) and res[4] == 1 and nc.satisfies(c, res[2])
        at = res[5]
        assert at >= 0 and all(cu == NOTHING for cu in res[7][at + 1:])                    # the later cubes load 0 and do not start
        for s in range(2):
            got = sm.interleaved(n, c, h, zero, None, 0, 4, seed=s, width=8)
            assert got[:2] == (1, 0) and nc.satisfies(c, got[2]) and got[4] >= 1
        met += 1
    assert met > 50


def test_instances_without_a_model_and_bad_penalties_at_every_depth():
    inst, hints, pens = nc.small()
    none = [(i, h, p) for i, h, p in zip(inst, hints, pens) if nc.any_model(*i) is None and sum(len(x) for x in i[1]) > 0]
    assert len(none) > 20
    for depth in range(0, 7):
        for (n, c), h, p in none[::3]:
            res = sm.sequential(n, c, h, p, None, 0, depth)
            assert res[:2] == (0, -1) and not res[2].any() and res[4] == 0 and res[5] == -1 and all(cu[0] == 1 for cu in res[7])
            assert sm.interleaved(n, c, h, p, None, 0, depth, seed=depth)[:2] == (0, -1)
        for (n, c), h, p in list(zip(inst, hints, pens))[5::40]:
            for wrong in (-1, nm.MAX_PENALTY + 1):
                q = np.array(p, dtype=np.int64)
                q[len(q) // 2] = wrong
                res = sm.sequential(n, c, h, q, h, 0, depth)
                assert res[:2] == (-3, 0) and not res[2].any() and res[3:7] == (0, 0, -1, -1)
                assert res[7] == [NOTHING] * (1 << depth)


def test_start_models():
    inst, hints, pens = nc.small()
    rng = np.random.RandomState(77)
    met = better = ignored = 0
    for (n, c), h, p in zip(inst, hints, pens):
        want = nm.search(n, c, h, p)
        m = nc.any_model(n, c)
        nn = len(want[2])
        bits, pen = nm.threshold(nn, h), nm.penalty_list(nn, p)
        for depth in (0, 2, 4):
            runs = []
            if m is not None:
                # a model: the same cost, start_cost its distance
                res = sm.sequential(n, c, h, p, m, 0, depth)
                assert res[:2] == want[:2] and res[6] == (nm.distance(bits, pen, m)) and res[1] <= res[6]
                runs.append(res)
                better += res[1] < res[6]
                # the optimum itself: nothing improves on it and it comes back
                res = sm.sequential(n, c, h, p, want[2], 0, depth)
                assert res[:2] == want[:2] and res[4] == 0 and res[5] == -1 and res[6] == want[1] and all(cu[2] == sm.NO_COST for cu in res[7])
                assert np.array_equal(res[2], want[2]) or want[1] == 0
                runs.append(res)
                runs.append(sm.interleaved(n, c, h, p, m, 0, depth, seed=depth, width=5))
                assert runs[-1][:2] == want[:2]
                met += 1
            # a non-model is ignored: the outputs of the call without one, but for the reads of its pass
            bad = rng.randint(0, 2, size=nn).astype(np.float32)
            if not nc.satisfies(c, bad):
                res, base = sm.sequential(n, c, h, p, bad, 0, depth), sm.sequential(n, c, h, p, None, 0, depth)
                assert res[6] == -1 and res[:3][:2] == base[:2] and np.array_equal(res[2], base[2]) and res[4:6] == base[4:6]
                assert res[7] == base[7] and res[3] > base[3]
                ignored += 1
            for r in runs:
                sc.attains((n, c), h, p, r)
    assert met > 300 and better > 50 and ignored > 300


def test_the_pinned_flip_prune():
    "fan_case at depth 2: cube 2 and 3 pin x1 against the hint at k + 5 > k, the cost cube 0 has found, and end before any pass"
    (n, clauses), hint, pen = nc.fan_case()
    want = nm.search(n, clauses, hint, pen)
    res = sm.sequential(n, clauses, hint, pen, None, 0, 2)
    assert res[:2] == want[:2] == (1, n - 1) and res[5] == 0
    sc.attains((n, clauses), hint, pen, res)
    first_pass = sum(len(c) for c in clauses)
    # one pass (no unit) and one branching pass (every clause has the minimum width and is read twice), and no pass behind the pin
    assert res[7][2] == res[7][3] == (1, 3 * first_pass, sm.NO_COST, 0)
    assert res[7][0][2:] == (n - 1, 1) and res[7][1][2:] == (sm.NO_COST, 0) and res[7][1][1] > 3 * first_pass
    # with the cost already known (the optimum as the start model) cubes 0 and 1 are pruned by the units instead, and nothing improves
    again = sm.sequential(n, clauses, hint, pen, want[2], 0, 2)
    assert again[:2] == want[:2] and again[5] == -1 and again[4] == 0 and again[7][2] == res[7][2] and np.array_equal(again[2], want[2])


def test_budget_is_per_cube():
    inst, hints, pens = nc.small()
    uni = nc.uniform()
    cases = list(zip(inst[::9], hints[::9], pens[::9])) + [(uni[0][k], uni[1][k], uni[2][k]) for k in (0, 7)]
    seen = set()
    for (n, c), h, p in cases:
        edges = sum(len([l for l in x if int(l) != 0]) for x in c)
        chk = sm.check(n, c, h, p)[4]
        for depth in (0, 2, 4):
            for sched in (0, 1):
                last = None
                for budget in (50, 500, 5000):
                    res = sm.sequential(n, c, h, p, None, budget, depth) if sched == 0 else \
                        sm.interleaved(n, c, h, p, None, budget, depth, seed=budget + depth)
                    status, cost, model, work, _, first, _, cubes = res
                    sc.attains((n, c), h, p, res)                                 # also under status -1
                    assert status == (-1 if any(cu[0] != 1 for cu in cubes) else (1 if cost >= 0 else 0))
                    assert all(cu[1] < budget + 3 * edges for cu in cubes)
                    assert all(chk + cu[1] >= budget for cu in cubes if cu[0] == -1)
                    assert work == chk + sum(cu[1] for cu in cubes) and work < chk + len(cubes) * (budget + 3 * edges)
                    if sched == 0 and last is not None and last[1] >= 0:
                        assert 0 <= cost <= last[1]                               # one schedule: a larger budget never finds a worse cost
                    last = res
                    seen.add(status)
    assert seen == {-1, 0, 1}


def test_the_uniform_instances():
    inst, hints, pens = nc.uniform()
    for k, ((n, c), h, p) in enumerate(zip(inst, hints, pens)):
        if n > 30:
            continue
        want = nm.search(n, c, h, p)
        assert want[0] in (0, 1)
        for depth in (2, 4):
            for res in (sm.sequential(n, c, h, p, None, 0, depth), sm.interleaved(n, c, h, p, None, 0, depth, seed=k, width=16)):
                assert res[:2] == want[:2]
                sc.attains((n, c), h, p, res)


@pytest.mark.parametrize('variant', sc.VARIANTS)
def test_the_gpu_batch_finishes_on_the_model(variant):
    "every instance of the GPU tests' batch, at its depth, ends proved far below the default budget, with the plain statement's cost"
    inst, _, _, depth = sc.batch()
    hints, pens, begin = sc.dressed(variant)
    assert 400 < len(inst) < 500 and set(depth.tolist()) == set(range(7)) and 2000 < int((1 << depth.astype(np.int64)).sum()) < 10000
    want = sc.batch_plain(variant)
    for j, res in enumerate(sc.batch_sequential(variant)):
        assert res[0] == want[0][j] and res[1] == want[1][j] and res[0] in (0, 1)
        assert all(cu[0] == 1 and cu[1] < (1 << 22) for cu in res[7])
        sc.attains(inst[j], hints[j], None if pens is None else pens[j], res)


def test_header_and_symbols():
    from pdp import native
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    assert '#define PDP_ABI_VERSION 3' in text
    assert ("int pdp_exact_nearest_split(pdp_problem *p, const float *hint, const int32_t *penalty, const float *start, const int8_t *depth, "
            "int64_t budget, int8_t *status, int64_t *cost, float *model, int64_t *work, int32_t *improvements, int32_t *first, "
            "int8_t *depth_used, int64_t *start_cost, void *stream);") in text
    assert ("int pdp_exact_nearest_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int64_t *cube_cost, int64_t *cube_work, "
            "int32_t *cube_improvements, void *stream);") in text
    assert re.search(r'pdp_exact_nearest_split, pdp_exact_nearest_split_cubes and pdp_exact_last_grid are additions[^/]*the version stays 3', text)
    assert {'pdp_exact_nearest_split', 'pdp_exact_nearest_split_cubes'} <= set(native.EXPORTED_SYMBOLS)
    assert 'exact_nearest_split' in native.Problem.exact_last_grid.__doc__
    assert re.search(r'the workgroups of the last launch that[^/]*pdp_exact_nearest_split', text)


@pytest.mark.parametrize('split', [17, -1, True, 'x', 2.0])
def test_nearest_model_refuses_a_bad_split(split):
    from pdp import exact
    with pytest.raises(ValueError, match='split must be'):
        exact.nearest_model([exact.raw_item(2, [[1, 2]])], None, split=split)
