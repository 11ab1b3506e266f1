"""The Python statements of proof logging and proof checking (tests/exact_proof_model.py; pdp_exact_solve_learn_proof and pdp_exact_check in
include/pdp_hip.h) on the CPU: the logging search is the learning model, genuine proofs verify and a verified proof means brute force
finds no model, forged proofs of satisfiable instances never verify, the mutation set the GPU test uses has both outcomes, the DRAT text,
and the wide families reach lemmas and proofs past one wave's width."""
import collections
import os
import sys

import numpy as np
import pytest

import exact_learn_model as lm
import exact_proof_model as pm
import exact_wide
from helpers import REPO
from test_exact_host import brute_force

ARENAS = (0, 12, 40)


def test_logging_search_equals_the_learning_model():
    inst, runs = pm.base_inputs()
    for A in ARENAS:
        got, want = runs[A], lm.solve(inst, arena=A)
        for k in (0, 2, 3, 4):
            np.testing.assert_array_equal(got[k], want[k])
        assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
        assert [len(x) for x in got[5]] == got[3].tolist()
        assert got[6].tolist() == [sum(len(l) + 1 for l in x) for x in got[5]]
    assert runs[40][4].any() and (runs[12][0] == -1).any()                           # reduced arenas, and lemmas that did not fit any more


@pytest.mark.parametrize('name', sorted(exact_wide.learn_batches()))
def test_logging_search_equals_the_learning_model_on_the_wide_batches(name):
    inst, arena, budget = exact_wide.learn_batches()[name]
    want = exact_wide.learn_results(name)[0]
    got = pm.solve(inst, budget=budget or pm.NO_BUDGET, arena=arena)
    for k in (0, 2, 3, 4):
        np.testing.assert_array_equal(got[k], want[k])
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and [len(x) for x in got[5]] == got[3].tolist()


def test_genuine_proofs_verify_and_verified_means_unsatisfiable():
    inst, runs = pm.base_inputs()
    small = 0
    for A in ARENAS:
        status, models, _, _, reductions, lemmas, plen = runs[A]
        unsat = np.nonzero(status == 0)[0]
        assert len(unsat) > 100 and (A == 0 or reductions[unsat].any())
        for i in unsat:
            n, c = inst[i]
            w = pm.words(lemmas[i])
            assert len(w) == plen[i]
            assert pm.check(n, c, 0, models[i], w, len(w))[:2] == (1, -1)
            if max([n] + [abs(l) for x in c for l in x]) <= 16:
                small += 1
                assert not brute_force(n, c)
        # the models verify as well, and the regions of undecided instances are not looked at
        for i in np.nonzero(status == 1)[0][::5]:
            assert pm.check(inst[i][0], inst[i][1], 1, models[i], pm.words(lemmas[i]), plen[i])[:2] == (1, -1)
        assert pm.check(inst[0][0], inst[0][1], -1, models[0], pm.words([]), 0) == (-1, -1, 0)
    assert small > 300


def test_incomplete_proofs_are_not_judged():
    inst, runs = pm.base_inputs()
    status, models, _, _, _, lemmas, plen = runs[0]
    i = int(np.argmax(plen))
    n, c = inst[i]
    assert status[i] == 0 and len(lemmas[i]) > 2
    cut = pm.region(lemmas[i], plen[i] // 2)
    assert 0 < len(cut) < plen[i] and np.array_equal(cut, pm.words(lemmas[i])[:len(cut)])
    assert pm.check(n, c, 0, models[i], cut, plen[i]) == (-1, -1, 0)
    assert pm.check(n, c, 0, models[i], pm.words(lemmas[i]), -1) == (-1, -1, 0)


def forged(n, clauses, lemmas):
    "the forged proofs of a satisfiable instance: the empty one, its own lemma log, and [x], [not x] on its first variable"
    return [[], lemmas, [[0], [1]]]


def test_forged_proofs_of_satisfiable_instances_never_verify():
    inst, runs = pm.base_inputs()
    seen = 0
    for A in ARENAS:
        status, models, _, learned, _, lemmas, _ = runs[A]
        for i in np.nonzero(status == 1)[0]:
            n, c = inst[i]
            for proof in forged(n, c, lemmas[i]):
                w = pm.words(proof)
                verdict, fail_at, _ = pm.check(n, c, 0, models[i], w, len(w))
                assert verdict == 0 and 0 <= fail_at <= len(proof)
                seen += 1
        assert learned[status == 1].any()                                             # a log of its own that is not empty
    assert seen > 300


def test_malformed_words_are_refuted_at_their_lemma():
    n, c = lm.thrash(4)
    lemmas = pm.search(n, c)[5]
    assert len(lemmas) == 3
    w = pm.words(lemmas)
    assert pm.check(n, c, 0, None, w, len(w))[:2] == (1, -1)
    at = len(lemmas[0]) + 1                                                          # the length word of lemma 1
    for word, pos in ((n << 1, at + 1), (-2, at + 1), (len(w), at), (-1, at)):       # a variable past n, a negative code, two bad lengths
        bad = w.copy()
        bad[pos] = word
        assert pm.check(n, c, 0, None, bad, len(bad))[:2] == (0, 1)


def test_mutation_set_has_both_outcomes():
    cases = pm.mutation_cases()
    cnt = collections.Counter((c['kind'], int(c['verdict'])) for c in cases)
    runs = cnt[('genuine', 1)]
    print({k: cnt[k] for k in sorted(cnt)})
    assert runs >= 40 and cnt[('genuine', 0)] == 0 and {c['arena'] for c in cases} == {0, 40}
    for kind in ('flip', 'shrink'):
        assert 4 * cnt[(kind, 0)] >= runs and 4 * cnt[(kind, 1)] >= runs
    for c in cases:
        if c['kind'] in ('empty', 'drop-first', 'reverse') and len(c['lemmas']) >= 2:
            assert c['verdict'] == 0
        assert c['verdict'] in (0, 1) and (c['fail_at'] == -1) == (c['verdict'] == 1)


def test_checker_budget_bound_and_decided_verdicts():
    cases = [c for c in pm.mutation_cases() if c['kind'] in ('genuine', 'flip')][::3]
    for c in cases:
        n, cl = c['inst']
        e, w = sum(len(x) for x in cl), pm.words(c['mutated'])
        for budget in (1, e, 10 * e):
            verdict, fail_at, work = pm.check(n, cl, 0, None, w, len(w), budget)
            assert work < budget + e + len(w)
            if verdict != -1:
                assert (verdict, fail_at, work) == (c['verdict'], c['fail_at'], c['work'])


def test_drat_lines():
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    from pdp import exact
    assert exact.drat_lines([]) == ['0']
    assert exact.drat_lines([[0, 3, 4], [5]]) == ['1 -2 3 0', '-3 0', '0']
    assert exact.proof_lemmas([3, 0, 3, 4, 1, 5, 0]) == [[0, 3, 4], [5], []]
    with pytest.raises(ValueError):
        exact.proof_lemmas([2, 0])
    n, c = lm.thrash(3)
    lemmas = pm.search(n, c)[5]
    lines = exact.drat_lines(lemmas)
    assert len(lines) == len(lemmas) + 1 and all(l.endswith('0') for l in lines)
    back = [[((abs(int(t)) - 1) << 1) | (int(t) < 0) for t in l.split()[:-1]] for l in lines[:-1]]
    assert back == lemmas


def test_wide_batches_reach_long_lemmas_and_long_proofs():
    "a lemma of more than 64 literals and a proof of more than 64 lemmas: what a wave handles in more than one step"
    stats = [s for name in exact_wide.learn_batches() for s in exact_wide.learn_results(name)[1]]
    learned = np.concatenate([exact_wide.learn_results(name)[0][3] for name in exact_wide.learn_batches()])
    assert exact_wide.peak(stats, 'lc') > 64 and learned.max() > 64


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    import satyr
    from pdp import generator
    with pytest.raises(SystemExit) as exc:
        satyr.main([os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml'), os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10',
                    '-d', '--complete-certify'])
    assert exc.value.code == 2 and '--complete-certify' in capsys.readouterr().err
    a = generator.cli_parser().parse_args(['o', 'j', 'n', '1', 'modular', '--certify'])
    assert a.certify and a.label == 'exact'
    assert not generator.cli_parser().parse_args(['o', 'j', 'n', '1', 'modular']).certify
    with pytest.raises(SystemExit):
        generator.main(['o', 'j', 'n', '1', 'modular', '--certify', '--label', 'none'])
    p = dimacs2json.cli_parser()
    a = p.parse_args(['in', 'out', '--label', 'exact-certified', '--proof-dir', 'd'])
    assert a.label == 'exact-certified' and a.proof_dir == 'd'
    assert p.parse_args(['in', 'out']).proof_dir is None
