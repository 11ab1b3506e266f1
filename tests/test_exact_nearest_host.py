"""The nearest-model search without a GPU: its Python statement (tests/exact_nearest_model.py) against an exhaustive minimum, the
consequences N1-N7 of the specification (include/pdp_hip.h) against the statements of the deciding and the counting search, the widths the
constructed instances of test_exact_nearest_gpu.py reach, exact.map_penalties, and the header."""
import os
import re

import numpy as np
import pytest

import exact_count_model as cm
import exact_model
import exact_nearest_cases as cs
import exact_nearest_model as nm
from helpers import REPO


def setting(i, n, hints, pens, mixed):
    return nm.threshold(n, hints[i]), nm.penalty_list(n, pens[i] if mixed else None)


def test_model_equals_brute_force():
    "a few hundred instances with n <= 12: widths 0 to 4, repeated literals, tautologies, empty clauses, unused variables, families.py"
    inst, hints, pens = cs.small()
    assert len(inst) > 400 and max(n for n, _ in inst) <= 12
    assert {int(q) for p in pens for q in p} == set(cs.MIXED)
    seen = set()
    for mixed in (True, False):
        st, cost, models, work, imp = cs.pick(cs.results(mixed), list(range(len(inst))))
        for i, (n, c) in enumerate(inst):
            bits, pen = setting(i, n, hints, pens, mixed)
            best, _ = cs.brute(n, c, bits, pen)
            if best is None:
                assert (st[i], cost[i], imp[i]) == (0, -1, 0) and not models[i].any()
                continue
            assert st[i] == 1 and cost[i] == best and models[i].shape == (n,) and set(np.unique(models[i])) <= {0.0, 1.0}
            assert cs.satisfies(c, models[i]) and nm.distance(bits, pen, models[i]) == best
            assert (imp[i] == 0) == cs.satisfies(c, bits)
            seen.add(min(int(imp[i]), 3))
    assert seen == {0, 1, 2, 3}


def test_n1_a_hint_that_is_a_model():
    inst, _, pens = cs.batch()
    hit = 0
    for i, (n, c) in enumerate(inst):
        m = cs.any_model(n, c)
        if m is None:
            continue
        st, cost, model, work, imp = nm.search(n, c, m, pens[i])
        assert (st, cost, imp) == (1, 0, 0) and np.array_equal(model, m)
        assert work == exact_model.search(n, c, m)[2]
        hit += 1
    assert hit > 200


def test_n2_n3_status_and_known_models():
    "status is the deciding search's; cost is at most the distance to the hinted search's model and to every model of the count's family"
    inst, hints, pens = cs.batch()
    for mixed in (True, False):
        st, cost, models, _, _ = cs.results(mixed)
        for i, (n, c) in enumerate(inst):
            bits, pen = setting(i, n, hints, pens, mixed)
            hs, hm, _ = exact_model.search(n, c, np.asarray(bits, dtype=np.float32))
            assert st[i] == hs == exact_model.search(n, c)[0]
            if st[i] == 1:
                assert cs.satisfies(c, models[i]) and cost[i] == nm.distance(bits, pen, models[i]) <= nm.distance(bits, pen, hm)


def test_n4_a_pruned_subtree_of_the_count():
    inst, hints, pens = cs.batch()
    edges = cs.edges(inst)
    count_work = np.array([cm.search(n, c)[3] for n, c in inst])
    for mixed in (True, False):
        work = cs.results(mixed)[3]
        assert (work <= count_work + edges).all()
    print('reads of the nearest-model search over the count\'s, uniform 3-SAT: %s'
          % np.round(cs.results(False)[3][len(cs.small()[0]):] / count_work[len(cs.small()[0]):], 2).tolist())


def test_n5_all_penalties_zero():
    inst, hints, _ = cs.batch()
    for i, (n, c) in enumerate(inst):
        st, cost, model, work, imp = nm.search(n, c, hints[i], np.zeros(n, dtype=np.int32))
        assert st == cs.results(True)[0][i] and imp <= 1
        if st == 1:
            assert cost == 0 and cs.satisfies(c, model)
            if imp == 1:                                                                     # the first leaf ended it: the hinted search's reads
                assert work == exact_model.search(n, c, np.asarray(nm.threshold(n, hints[i]), dtype=np.float32))[2]


def test_n6_scaling_the_penalties():
    inst, hints, pens = cs.small()
    for i, (n, c) in enumerate(inst[:200]):
        q = np.minimum(pens[i], 7)
        a = nm.search(n, c, hints[i], q)
        for k in (3, 149796):
            b = nm.search(n, c, hints[i], q * k)
            assert b[1] == (a[1] * k if a[1] >= 0 else -1)
            assert (a[0], a[3], a[4]) == (b[0], b[3], b[4]) and np.array_equal(a[2], b[2])


def test_n7_budget_of_the_model():
    inst, hints, pens = cs.batch()
    full = cs.results(True)
    edges = cs.edges(inst)
    last, seen = None, set()
    for budget in (1, 50, 500, 5000):
        st, cost, models, work, imp = cs.results(True, budget)
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all()
        for i in np.nonzero((st == 0) | ((st == -1) & (cost == -1)))[0]:
            assert not models[i].any() and cost[i] == -1
        for i in np.nonzero(cost >= 0)[0]:
            n, c = inst[i]
            assert cs.satisfies(c, models[i]) and nm.distance(*setting(i, n, hints, pens, True), models[i]) == cost[i] >= full[1][i]
        assert (cost[st != -1] == full[1][st != -1]).all() and (st[st != -1] == full[0][st != -1]).all()
        if last is not None:
            assert (cost[last >= 0] >= 0).all() and (cost[last >= 0] <= last[last >= 0]).all()
        last = cost
        seen |= {(int(s), bool(c >= 0)) for s, c in zip(st, cost)}
    assert seen == {(1, True), (0, False), (-1, True), (-1, False)}


def test_refusal_of_a_penalty_out_of_range():
    for bad in (-1, cs.CAP + 1):
        st, cost, model, work, imp = nm.search(3, [[1, 2], [-1, 3]], None, [1, bad, 1])
        assert (st, cost, work, imp) == (-3, 0, 0, 0) and not model.any()
    assert nm.search(3, [[1, 2], [-1, 3]], None, [0, cs.CAP, 1])[0] == 1


def test_the_uniform_instances_finish_under_the_read_limit():
    inst, _, _ = cs.uniform()
    first = len(cs.small()[0])
    assert sorted({n for n, _ in inst}) == list(cs.UNIFORM_N)
    for mixed in (True, False):
        st, _, _, work, _ = cs.results(mixed)
        assert (st[first:] != -1).all() and (work[first:] < cs.READ_LIMIT).all()
        assert {0, 1} == set(st[first:][[n == 50 for n, _ in inst]])                          # n = 50: satisfiable and unsatisfiable


def test_widths_of_the_constructed_instances():
    "what test_exact_nearest_gpu.py's shapes reach in the model: chunks past 64 of a pass's sum, of an undo and of the leaf's fill"
    for case, key, least in ((cs.fan_case(150), 'pass_against', 150), (cs.units_case(4100), 'pass_against', 4100), (cs.fill_case(100), 'fill', 100)):
        stats = {}
        st, cost, model, _, _ = nm.search(*case[0], case[1], case[2], stats=stats)
        assert st == 1 and stats[key] >= least
    fan = {}
    assert nm.search(*cs.fan_case(150)[0], cs.fan_case(150)[1], cs.fan_case(150)[2], stats=fan)[1] == 150
    assert fan['undone'] > 128 and fan['flip_pruned'] == 1
    assert nm.search(*cs.units_case(4100)[0], cs.units_case(4100)[1], cs.units_case(4100)[2])[1] == 4100 << 20 > 1 << 32
    (st, cost, _, _, imp), stats = cs.wide_results()
    assert max(s.get('trail', 0) for s in stats) > 128 and max(s.get('pass_units', 0) for s in stats) >= 100
    assert max(s.get('undone', 0) for s in stats) > 64 and max(s.get('pass_against', 0) for s in stats) > 64
    assert (st == 1).any() and (st == -1).any() and (imp > 0).any()


def test_map_penalties():
    from pdp import exact
    h, q = exact.map_penalties([0.0, 0.5, 1.0, 0.5 + 2.0 ** -30, 0.9, 0.1, 0.75])
    assert h.dtype == np.float32 and q.dtype == np.int32
    assert h.tolist() == [0, 0, 1, 1, 1, 0, 1]
    assert q.tolist() == [cs.CAP, 0, cs.CAP, 0, 2250, 2250, 1125]                                # 1024 ln 9 = 2249.9, 1024 ln 3 = 1124.98
    h, q = exact.map_penalties(np.array([[0.9, 1e-300], [0.5, 0.6]]), scale=1 << 19)
    assert q.shape == (2, 2) and q.tolist() == [[cs.CAP, cs.CAP], [0, int(np.rint((1 << 19) * np.log(1.5)))]]
    for bad in ([0.2, np.nan], [-0.1], [1.0000001]):
        with pytest.raises(ValueError):
            exact.map_penalties(bad)
    with pytest.raises(ValueError):
        exact.map_penalties([0.5], scale=0)


def test_map_penalties_give_the_most_probable_model():
    "on small instances the nearest model under map_penalties has the highest probability under the product prior, up to the quantisation"
    from pdp import exact
    rng = np.random.RandomState(23)
    inst = cs.small()[0][:120]
    for n, c in inst:
        p = np.clip(np.round(rng.rand(n), 2), 0.01, 0.99)
        h, q = exact.map_penalties(p)
        st, cost, model, _, _ = nm.search(n, c, h, q)
        best, models = cs.brute(n, c, h, q)
        if best is None:
            continue
        logp = np.where(models, np.log(p), np.log1p(-p)).sum(axis=1)
        mine = np.where(model > 0.5, np.log(p), np.log1p(-p)).sum()
        assert cost == best and mine >= logp.max() - (n * 0.5 + 1e-9) / 1024                  # half a unit of rounding per variable


def test_header_declares_the_entry_point():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = f.read()
    assert re.search(r'int pdp_exact_nearest\(pdp_problem \*p, const float \*hint, const int32_t \*penalty, int64_t budget, int8_t \*status, '
                     r'int64_t \*cost,\s+float \*model, int64_t \*work, int32_t \*improvements, void \*stream\);', text)
    assert re.search(r'#define PDP_ABI_VERSION 3\b', text)
    from pdp import native
    assert 'pdp_exact_nearest' in native.EXPORTED_SYMBOLS
