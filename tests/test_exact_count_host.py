"""The counting complete search without a GPU: its Python statement (tests/exact_count_model.py) against brute-force enumeration, against
the deciding search's statement and the brute-force backbone, the budget rules, the cases where the doubles round, and the header."""
import os
import re

import numpy as np

import exact_count_cases as cs
import exact_count_model as cm
import exact_model
from helpers import REPO


def test_model_equals_brute_force():
    inst, want = cs.family(), cs.family_brute()
    assert len(inst) >= 300 and max(n for n, _ in inst) <= 12
    widths = {len(c) for _, cl in inst for c in cl}
    assert widths >= {0, 1, 2, 3, 4}
    assert any(len(set(c)) < len(c) for _, cl in inst for c in cl)                        # a repeated literal
    assert any(any(-l in c for l in c) for _, cl in inst for c in cl)                     # a tautology
    assert any(n > max([abs(l) for c in cl for l in c] + [0]) for n, cl in inst)          # an unused variable
    st, count, tcs, work, leaves = cm.solve(inst)
    assert (st == 1).all()
    print('counts: %d instances, %d with models, largest %d, most leaves %d' % (len(inst), int((count > 0).sum()), int(count.max()), int(leaves.max())))
    assert int((count > 0).sum()) >= 150 and int((count == 0).sum()) >= 30
    for (n, c), (bc, bt), co, tc, lv in zip(inst, want, count, tcs, leaves):
        assert tc.shape == (n,) and tc.dtype == np.float64
        assert co == float(int(co)) and int(co) == bc
        assert [int(x) for x in tc] == bt.tolist() and (tc == np.floor(tc)).all()
        assert (lv > 0) == (bc > 0) and lv <= max(bc, 0)


def test_agrees_with_the_deciding_search_and_the_backbone():
    inst, want = cs.family(), cs.family_brute()
    _, count, tcs, _, _ = cm.solve(inst)
    forced = 0
    for (n, c), (bc, bt), co, tc in zip(inst, want, count, tcs):
        assert (co > 0) == (exact_model.search(n, c)[0] == 1)
        if bc > 0:
            backbone = (bt == bc) | (bt == 0)
            np.testing.assert_array_equal((tc == co) | (tc == 0), backbone)
            forced += int(backbone.sum())
    assert forced > 100


def test_budget_of_the_model():
    inst = cs.family()[::4] + cs.uniform_3sat(3, 20, (3.5, 4.0), 5)
    full = cm.solve(inst)
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    last = None
    seen = set()
    for budget in (1, 50, 500, 5000):
        st, count, tcs, work, leaves = cm.solve(inst, budget)
        assert set(np.unique(st)) <= {-1, 1}
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all()
        assert (count <= full[1]).all() and (last is None or (count >= last).all())
        assert (leaves <= full[4]).all()
        for s, co, tc, fc, ft in zip(st, count, tcs, full[1], full[2]):
            assert (tc >= 0).all() and (tc <= co).all() and (tc <= ft).all()
            assert co == float(int(co)) and (tc == np.floor(tc)).all()                    # a partial count is a count of whole models
            if s == 1:
                assert co == fc and np.array_equal(tc, ft)
        if budget == 1:
            # the budget check fires after the first pass: nothing is counted unless that pass was everything
            assert (count[(st == -1)] == 0).all()
        last = count
        seen |= set(np.unique(st))
        if budget == 500:
            assert ((st == -1) & (count > 0)).any()                                       # a lower bound that is not trivial
    assert seen == {-1, 1} and (st == 1).any()


def test_counts_that_round():
    from pdp import exact
    for k in cs.FAN_K:
        n, clauses = cs.fan(k)
        st, count, tc, work, leaves = cm.search(n, clauses)
        assert (st, leaves) == (1, 2)
        assert count == 2.0 ** k                                                          # 2^k + 1, rounded
        assert tc[0] / count == 1.0 and (tc[1:] / count == 0.5).all()
        assert not exact.count_is_exact(np.array([st]), np.array([count]))[0]
    assert exact.count_is_exact(np.array([1, -1, 1, -2]), np.array([2.0 ** 53, 5.0, 2.0 ** 53 + 2, 0.0])).tolist() == [True, False, False, False]
    stats = {}
    cm.search(*cs.fan(150), stats=stats)
    assert stats['pass_units'] == 150 and stats['undone'] == 151 and stats['trail'] == 151    # one level past two chunks of 64


def test_unused_variables_double_the_count():
    (n, clauses), core = cs.padded_core(60)
    st, count, tc, _, _ = cm.search(n, clauses)
    assert st == 1 and core > 0 and count == core * 2.0 ** 60
    bc, bt = cs.brute(12, clauses)
    assert bc == core
    np.testing.assert_array_equal(tc[:12], bt * 2.0 ** 60)
    assert (tc[12:] == count * 0.5).all()


def test_too_many_variables():
    st, count, tc, work, leaves = cm.search(1024, [[1, 2], [-1, 1024]])
    assert (st, count, work, leaves) == (-2, 0.0, 0, 0) and tc.shape == (1024,) and not tc.any()
    st, count, tc, _, _ = cm.search(1023, [[1, 2], [-1, 1023]])
    assert st == 1 and count == 2.0 ** 1021 * 2 and np.isfinite(tc).all()                 # 4 of 8 over three variables


def test_case_past_the_slab():
    n, clauses = cs.past_the_slab()
    st, count, tc, _, leaves = cs.slab_result()
    assert cs.slab_bytes(n, len(clauses), sum(len(c) for c in clauses)) > cs.LDS_LIMIT
    bc, bt = cs.brute(n, clauses)
    assert st == 1 and count == bc >= 20 and tc.tolist() == bt.tolist() and leaves >= 5


def test_header_and_symbol():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = f.read()
    assert '#define PDP_ABI_VERSION 3' in text
    proto = ("int pdp_exact_count(pdp_problem *p, int64_t budget, int8_t *status, double *count, double *true_count, int64_t *work, "
             "int64_t *leaves, void *stream);")
    assert proto in re.sub(r'\s+', ' ', text)
    from pdp import native
    assert 'pdp_exact_count' in native.EXPORTED_SYMBOLS
