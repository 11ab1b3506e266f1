"""The specification of the learning complete search (tests/exact_learn_model.py; pdp_exact_solve_learn in include/pdp_hip.h) on the CPU:
equal to brute force on small instances of every degenerate kind at three arena sizes, the "thrash" family that chronological
backtracking cannot handle, the work bound, and the command-line flags that select the search."""
import os
import sys

import numpy as np
import pytest

import exact_learn_model as lm
import exact_model
from helpers import REPO
from test_exact_host import brute_force, dpll

ARENAS = (lm.NO_ARENA, 40, 12)            # unlimited; reached by reductions; exhausted by some instances


def satisfies(clauses, model):
    return all(any((model[abs(l) - 1] > 0.5) == (l > 0) for l in c) for c in clauses)


def small_instances(count=420, seed=61):
    """n <= 12, clauses of 1 to 3 literals.  Two instances in three are near the 3-SAT threshold (8 to 12 variables, 3 n to 5.5 n clauses, nine
    in ten of them on three distinct variables) so that conflicts above level 0 occur; the others have 1 to 12 variables and any density.
    The remaining clauses are drawn with replacement (repeated literals, tautologies) with 4 % units, and every 30th instance has an empty clause."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        hard = i % 3 != 0
        n = int(rng.randint(8, 13)) if hard else int(rng.randint(1, 13))
        m = int(rng.randint(3 * n, int(5.5 * n) + 1)) if hard else int(rng.randint(1, int(5.5 * n) + 2))
        clauses = []
        for _ in range(m):
            if hard and rng.rand() < 0.9:
                vs = rng.choice(n, size=3, replace=False) + 1
            else:
                vs = rng.randint(1, n + 1, size=int(rng.choice([1, 2, 3], p=[0.04, 0.26, 0.7])))
            clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=len(vs)))])
        if i % 30 == 29:
            clauses.insert(int(rng.randint(0, len(clauses) + 1)), [])
        out.append((n, clauses))
    return out


def edges(inst):
    return np.array([sum(len(c) for c in cl) for _, cl in inst], dtype=np.int64)


@pytest.fixture(scope='module')
def small():
    inst = small_instances()
    return inst, np.array([brute_force(n, c) for n, c in inst]), {A: lm.solve(inst, arena=A) for A in ARENAS}


def test_small_instances_have_every_degenerate_kind():
    inst = small_instances()
    flat = [c for _, cl in inst for c in cl]
    assert len(inst) >= 400
    assert any(len(c) == 0 for c in flat) and any(len(c) == 1 for c in flat)
    assert any(len(c) != len(set(c)) for c in flat)                                  # a repeated literal
    assert any(any(-l in c for l in c) for c in flat)                                # a tautology


def test_model_equals_brute_force(small):
    inst, want, runs = small
    assert 100 < int(want.sum()) < len(inst) - 100
    for A in ARENAS:
        status, models, work, learned, reductions = runs[A]
        decided = status != -1
        np.testing.assert_array_equal(status[decided] == 1, want[decided])           # never a wrong answer
        assert all(satisfies(c, m) for (n, c), s, m in zip(inst, status, models) if s == 1)
        assert all(len(m) == n and not m.any() for (n, c), s, m in zip(inst, status, models) if s != 1)
        if A == lm.NO_ARENA:
            assert decided.all() and not reductions.any()                            # undecided only with a finite arena
            assert int((learned > 0).sum()) > 100
    assert runs[12][4].any(), "the 12-word arena is never reduced"


def test_family_instances_reach_reduction_and_exhaustion():
    "families.exact_cases(): the default arena decides them all as the reference DPLL does; 40 words are reduced, 12 words run out"
    import families
    inst = [(n, c) for _, n, c in families.exact_cases()]
    want = np.array([dpll(n, c) for n, c in inst])
    for A in (0, 40, 12):
        status, models, work, learned, reductions = lm.solve(inst, arena=A)
        decided = status != -1
        np.testing.assert_array_equal(status[decided] == 1, want[decided])
        assert all(satisfies(c, m) for (n, c), s, m in zip(inst, status, models) if s == 1)
        if A == 0:
            assert decided.all() and not reductions.any() and learned.max() > 40
        else:
            assert reductions.any() and (A == 40 or int((~decided).sum()) >= 3)
            assert (work < exact_model.NO_BUDGET).all() and (work[~decided] > 0).all()


def test_work_bound(small):
    inst, _, runs = small
    e = edges(inst)
    for A in (40, 12, 0):
        words = 4 * e if A == 0 else A
        full = runs[A] if A else lm.solve(inst)
        for budget in (1, 30, 300):
            status, _, work, _, _ = lm.solve(inst, budget=budget, arena=A)
            assert (work < budget + 4 * (e + words)).all()
            done = status != -1
            np.testing.assert_array_equal(status[done], full[0][done])
            np.testing.assert_array_equal(work[done], full[2][done])


def test_no_hints_and_own_model_as_hint(small):
    inst, _, runs = small
    status, models, work, learned, _ = runs[lm.NO_ARENA]
    for i in range(0, len(inst), 7):
        n, c = inst[i]
        nan = lm.search(n, c, hints=np.full(n, np.nan), arena=lm.NO_ARENA)
        assert (nan[0], nan[2], nan[3]) == (status[i], work[i], learned[i]) and np.array_equal(nan[1], models[i])
        if status[i] == 1:
            own = lm.search(n, c, hints=models[i], arena=lm.NO_ARENA)
            assert own[0] == 1 and np.array_equal(own[1], models[i]) and own[3] == 0
            assert own[2] == exact_model.check_reads([[l for l in x] for x in c], models[i])[0]


def test_thrash_family():
    "chronological backtracking refutes the last three variables under every combination of the k decisions before them; learning does it once"
    reads = []
    for k in (2, 4, 6, 8, 10, 12):
        n, clauses = lm.thrash(k)
        status, _, work, learned, _ = lm.search(n, clauses)
        assert status == 0 and learned == 3
        reads.append(work)
    assert reads == [472, 662, 884, 1138, 1424, 1742]
    n, clauses = lm.thrash(12)
    assert n == 27 and reads[-1] < 10_000
    status, _, work = exact_model.search(n, clauses)
    assert status == 0 and work > 2_000_000


def test_cli_flags(capsys):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    import satyr
    from pdp import generator
    with pytest.raises(SystemExit) as exc:
        satyr.main([os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml'), os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10',
                    '-d', '--complete-learn'])
    assert exc.value.code == 2 and '--complete-learn' in capsys.readouterr().err
    a = generator.cli_parser().parse_args(['o', 'j', 'n', '1', 'modular', '--learn'])
    assert a.learn and a.label == 'exact'
    assert not generator.cli_parser().parse_args(['o', 'j', 'n', '1', 'modular']).learn
    with pytest.raises(SystemExit):
        generator.main(['o', 'j', 'n', '1', 'modular', '--learn', '--label', 'none'])
    p = dimacs2json.cli_parser()
    assert p.parse_args(['in', 'out', '--label', 'exact-learn']).label == 'exact-learn'
    assert p.parse_args(['in', 'out']).label == 'name'
