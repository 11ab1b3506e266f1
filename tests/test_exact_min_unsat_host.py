"""The optimising complete search without a GPU: its Python statement (tests/exact_min_unsat_model.py) against an exhaustive minimum,
property M1 of the specification (include/pdp_hip.h) against the hinted deciding search's statement, the widths the constructed
instances of test_exact_min_unsat_gpu.py reach, and the header."""
import os
import re

import numpy as np

import exact_min_unsat_cases as cs
import exact_min_unsat_model as mm
import exact_model
from helpers import REPO


def test_model_equals_brute_force():
    inst, kinds = cs.family(11, 300, 11)
    want = np.array([cs.brute_min(n, c) for n, c in inst])
    hist = np.bincount(want)
    print('optimum histogram', hist.tolist())
    assert (hist[:5] >= 20).all()                                        # the family alone covers the optima 0 .. 4
    for k in cs.KINDS:
        st, cost, models, work, imp = mm.solve(inst, kinds[k])
        assert (st == 1).all()
        np.testing.assert_array_equal(cost, want)
        for (n, c), m, co, h, i in zip(inst, models, cost, kinds[k], imp):
            assert m.shape == (n,) and set(np.unique(m)) <= {0.0, 1.0}
            assert mm.unsat_count(c, m) == co
            first = mm.unsat_count(c, mm.threshold(n, h))
            assert co <= first and (i > 0) == (co < first)
            if i == 0:
                assert np.array_equal(m, np.asarray(mm.threshold(n, h), dtype=np.float32))


def test_budget_of_the_model():
    inst, kinds = cs.family(12, 60, 11)
    full = mm.solve(inst, kinds['random'])
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    last = None
    for budget in (1, 60, 600):
        st, cost, models, work, _ = mm.solve(inst, kinds['random'], budget)
        assert set(np.unique(st)) <= {-1, 1} and (work < budget + 3 * edges).all()
        assert (cost >= full[1]).all() and (cost[st == 1] == full[1][st == 1]).all()
        assert all(mm.unsat_count(c, m) == co for (_, c), m, co in zip(inst, models, cost))
        assert last is None or (cost <= last).all()
        last = cost
    assert (st == -1).any() and (st == 1).any()


def test_m1_against_the_hinted_search():
    "3-SAT n = 30, m = 138; the hint is a model of the instance without its last clause, so it leaves at most that one unsatisfied"
    rng = np.random.RandomState(5)
    seen = {0: 0, 1: 0}
    for _ in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 138)
        s, hint, _ = exact_model.search(n, clauses[:-1])
        if s != 1:
            continue
        first = mm.unsat_count(clauses, hint)
        assert first <= 1
        want = exact_model.search(n, clauses, hint)
        st, cost, model, work, _ = mm.search(n, clauses, hint)
        assert st == 1 and work == want[2]
        assert cost == (0 if want[0] == 1 else first)
        seen[want[0]] += 1
        if first == 1 and want[0] == 1:
            assert np.array_equal(model, want[1])                       # the same search found the same model
    print('M1: hinted search answered 1 on %d and 0 on %d instances' % (seen[1], seen[0]))
    assert seen[0] >= 1 and seen[1] >= 5


def test_wide_instances_reach_their_widths():
    for F in cs.WIDE_F:
        (n, clauses), hint = cs.wide(F)
        (st, cost, model, work, imp), stats = cs.wide_results(F)
        print('wide(%d): n %d m %d work %d improvements %d stats %s' % (F, n, len(clauses), work, imp, stats))
        assert n > 128 and len(clauses) > 128
        assert mm.unsat_count(clauses, hint) == 3
        assert (st, cost) == (1, 2) and imp >= 1 and mm.unsat_count(clauses, model) == 2
        assert stats['pass_units'] > 64                                  # a pass that forces more than 64 units
        assert stats['trail'] > 128                                      # a trail past 128
        assert stats['pass_cost'] > 64                                   # more than 64 clauses falsified in one pass
        assert stats['unit_branch'] == 1                                 # a branch on a width-1 clause
        plain = mm.search(n, clauses, hint)
        assert plain[:2] == (st, cost) and plain[3:] == (work, imp) and np.array_equal(plain[2], model)


def test_case_past_the_slab():
    (n, clauses), hint = cs.past_the_slab()
    st, cost, model, work, imp = cs.slab_result()
    assert cs.slab_bytes(n, len(clauses), sum(len(c) for c in clauses)) > cs.LDS_LIMIT
    assert st == 1 and cost == cs.brute_min(n, clauses) >= 1 and mm.unsat_count(clauses, model) == cost and imp >= 1


def test_header_and_symbol():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = f.read()
    assert '#define PDP_ABI_VERSION 3' in text
    proto = ("int pdp_exact_min_unsat(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, int32_t *cost, float *model, "
             "int64_t *work, int32_t *improvements, void *stream);")
    assert proto in re.sub(r'\s+', ' ', text)
    from pdp import native
    assert 'pdp_exact_min_unsat' in native.EXPORTED_SYMBOLS
