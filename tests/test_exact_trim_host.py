"""The backward check of a proof in plain Python (tests/exact_trim_model.py, the statement of pdp_exact_trim) against the searches and the
forward checker: every core is unsatisfiable on its own (T3), the kept lemmas are a proof against the core alone (T4), a proof the forward
check accepts is accepted (T1, T2), forged proofs, the work bound, the budget, malformed lemmas, the branches the shared inputs reach, and
the size of the cores on the community-attachment family."""
import numpy as np
import pytest

import exact_model
import exact_proof_model as pm
import exact_trim_model as tm


def holds_t3_t4(inst, region, plen, core, keep_lemmas):
    "the core alone is refuted by the plain search, and the forward checker accepts the kept lemmas against the core alone"
    sub = tm.core_instance(inst, core)
    assert exact_model.search(sub[0], sub[1])[0] == 0
    w = pm.words(tm.kept(region, plen, keep_lemmas))
    assert pm.check(sub[0], sub[1], 0, None, w, len(w))[:2] == (1, -1)


def lemma_marks(region, plen, keep):
    "keep words -> one 0/1 per lemma"
    out, pos = [], 0
    while pos < plen:
        out.append(int(keep[pos]))
        assert (keep[pos:pos + 1 + int(region[pos])] == keep[pos]).all()
        pos += 1 + int(region[pos])
    return out


def test_base_inputs_cores_and_trimmed_proofs():
    inst, regions, plen, want, _ = tm.base_cases()
    verdict, fail_at, work, cores, keeps, n_core, n_keep = want
    assert len(inst) > 500 and (verdict == 1).all() and (fail_at == -1).all()
    for b in range(len(inst)):
        marks = lemma_marks(regions[b], plen[b], keeps[b])
        assert n_core[b] == cores[b].sum() and n_keep[b] == sum(marks)
        holds_t3_t4(inst[b], regions[b], plen[b], cores[b], marks)
    assert (n_core >= 1).all() and n_keep.max() > 30
    # some core is the whole instance, most are not
    m = np.array([len(c) for _, c in inst])
    assert (n_core == m).any() and (n_core < m).sum() > len(inst) // 2


def test_mutated_and_forged_proofs():
    inst, status, regions, plen, want, _, forward = tm.mutation_batch()
    verdict, fail_at, work, cores, keeps, n_core, n_keep = want
    assert set(np.unique(verdict)) == {-1, 0, 1}
    seen = {(f, int(v)) for f, v in zip(forward, verdict) if f is not None}
    assert (0, 1) in seen and (0, 0) in seen and (1, 1) in seen               # also a proof only the backward check accepts
    for b in range(len(inst)):
        if forward[b] == 1:
            assert verdict[b] == 1                                              # T1
        if verdict[b] == 0 and forward[b] is not None:
            assert forward[b] == 0                                              # T2
        if verdict[b] == 1:
            holds_t3_t4(inst[b], regions[b], plen[b], cores[b], lemma_marks(regions[b], plen[b], keeps[b]))
        else:
            assert not cores[b].any() and n_core[b] == 0 and n_keep[b] == 0 and (keeps[b] is None or not keeps[b].any())
        if status[b] != 0 or not 0 <= plen[b] <= len(regions[b]):
            assert (verdict[b], fail_at[b], work[b]) == (-1, -1, 0) and keeps[b] is None
    # T2 against the forward checker itself, on every judged instance
    for b in np.nonzero(verdict == 0)[0]:
        assert pm.check(inst[b][0], inst[b][1], 0, None, regions[b], int(plen[b]))[0] == 0
    # a satisfiable instance has no refutation, whatever the words say
    base, runs = pm.base_inputs()
    sat = {id(base[i]) for i in range(len(base)) if runs[0][0][i] == 1}
    forged = [b for b in range(len(inst)) if id(inst[b]) in sat]
    assert len(forged) >= 60 and all(verdict[b] == 0 for b in forged)


def test_work_bound_and_budget():
    inst, regions, plen, want, _ = tm.base_cases()
    pick = np.argsort(want[2])[-40:]                                            # the longest checks
    for b in pick:
        n, c = inst[b]
        e, W, full = sum(len(x) for x in c), len(regions[b]), int(want[2][b])
        for budget in (1, full // 3, full - 1, full):
            v, f, w, core, keep = tm.trim(n, c, regions[b], int(plen[b]), budget)
            assert w < budget + 3 * (e + W)
            if v == -1:
                assert f == -1 and 0 < w <= full and not any(core) and not any(keep)
            else:
                assert (v, f, w) == (1, -1, full) and np.array_equal(core, want[3][b])
        assert tm.trim(n, c, regions[b], int(plen[b]), 1)[0] == -1 and tm.trim(n, c, regions[b], int(plen[b]), full // 3)[0] == -1
        assert tm.trim(n, c, regions[b], int(plen[b]), full)[0] == 1          # the last check of the budget comes before the last pass


@pytest.mark.parametrize('kind', tm.MALFORMED)
def test_malformed_lemmas(kind):
    cases = [c for c in pm.mutation_cases() if c['kind'] == 'genuine' and len(c['lemmas']) >= 3][:10]
    assert len(cases) == 10
    for c in cases:
        n, clauses = c['inst']
        for at in (0, len(c['lemmas']) // 2, len(c['lemmas']) - 1):
            w = tm.malform(c['inst'], c['lemmas'], kind, at)
            v, f, work, core, keep = tm.trim(n, clauses, w, len(w))
            assert (v, f, work) == (0, at, 0) and not any(core) and keep is None
            # the forward checker meets it when it arrives there, with the reads up to it counted
            fv = pm.check(n, clauses, 0, None, w, len(w))
            assert fv[:2] == (0, at) and (fv[2] > 0 or at == 0)


def test_inputs_reach_every_branch():
    for stats in (tm.base_cases()[4], tm.mutation_batch()[5], tm.wide_cases()[4]):
        for key in ('start-falsified', 'start-both', 'skipped', 'closure-lemma', 'closure-originals'):
            assert stats.get(key, 0) > 0, key
    # A lemma with both polarities of a variable is never falsified and never asks for a literal, so nothing marks it: the rule "accepted,
    # with no antecedents" of the forward checker is unreachable backwards.  The inputs hold such lemmas, needed by nobody.
    inst, status, regions, plen, want, stats, _ = tm.mutation_batch()
    found = 0
    for b in np.nonzero(want[0] == 1)[0]:
        for lemma, k in zip(pm.parse(regions[b][:plen[b]]), lemma_marks(regions[b], plen[b], want[4][b])):
            if any(L ^ 1 in lemma for L in lemma):
                found += 1
                assert k == 0
    assert found >= 10
    # past one wave's width
    wide = tm.wide_cases()[4]
    assert wide['peak-batch'] > 128 and wide['peak-antecedent'] > 128 and wide['peak-checked-lemma'] > 128 and wide['peak-lemmas'] > 128
    assert tm.wide_cases()[3][6].max() > 128 and (tm.wide_cases()[3][0] == 1).all()


def test_modular_cores_are_small():
    inst = tm.modular()
    run = pm.solve(inst)
    unsat = np.nonzero(run[0] == 0)[0]
    assert len(inst) == 8 and len(unsat) >= 4
    for i in unsat:
        n, c = inst[i]
        w = pm.words(run[5][i])
        v, f, work, core, keep = tm.trim(n, c, w, len(w))
        forward = pm.check(n, c, 0, None, w, len(w))
        sub = tm.core_instance(inst[i], core)
        kw = pm.words(tm.kept(w, len(w), keep))
        small = pm.check(sub[0], sub[1], 0, None, kw, len(kw))
        print("modular n = 60: core %d of %d clauses, %d of %d lemmas kept, backward %d reads, forward %d, forward on (core, kept) %d"
              % (sum(core), len(c), sum(keep), len(keep), work, forward[2], small[2]))
        assert v == 1 and forward[0] == 1 and small[:2] == (1, -1)
        assert 4 * sum(core) < len(c)
        assert exact_model.search(sub[0], sub[1])[0] == 0
