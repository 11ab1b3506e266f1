"""The Python statement of the hinted complete search (tests/exact_model.py, the specification of pdp_exact_solve_hinted) against brute
force, and the four properties the GPU tests rely on.  No GPU needed."""
import numpy as np
import pytest

import exact_model
from test_exact_gpu import DEGENERATE, random_instance, satisfies
from test_exact_host import brute_force


def hint_kinds(rng, inst, own):
    "per instance: random 0/1, random with 30 % NaN, the unhinted run's own model"
    rnd = [rng.randint(0, 2, size=n).astype(np.float32) for n, _ in inst]
    holes = []
    for n, _ in inst:
        h = rng.rand(n).astype(np.float32)
        h[rng.rand(n) < 0.3] = np.nan
        holes.append(h)
    return {'random': rnd, 'nan30': holes, 'own': [m.copy() for m in own]}


@pytest.fixture(scope='module')
def batch():
    rng = np.random.RandomState(515)
    inst = [random_instance(rng, 12) for _ in range(400)] + DEGENERATE
    plain = exact_model.solve(inst)
    kinds = hint_kinds(rng, inst, plain[1])
    return inst, plain, {k: exact_model.solve(inst, h) for k, h in kinds.items()}, kinds


def test_model_equals_brute_force_under_every_hint_kind(batch):
    inst, plain, hinted, _ = batch
    want = np.array([brute_force(n, c) for n, c in inst])
    assert 50 < int(want.sum()) < len(inst) - 50
    for status, models, _ in [plain] + list(hinted.values()):
        np.testing.assert_array_equal(status == 1, want)                 # P1: hints never change the status
        for (n, c), s, m in zip(inst, status, models):
            assert m.shape == (n,) and set(np.unique(m)) <= {0.0, 1.0}
            assert satisfies(c, m) if s == 1 else not m.any()


def test_unsat_work_is_unhinted_plus_check_reads(batch):
    "P2"
    inst, plain, hinted, kinds = batch
    seen = 0
    for k in ('random', 'nan30'):
        for i, (n, c) in enumerate(inst):
            if plain[0][i] != 0:
                continue
            h = kinds[k][i]
            extra = 0 if np.isnan(h).any() else exact_model.check_reads(c, h)[0]
            assert hinted[k][2][i] == plain[2][i] + extra
            seen += extra > 0
    assert seen > 50


def test_own_model_is_accepted_by_the_check_pass(batch):
    "P3"
    inst, plain, hinted, _ = batch
    for i, (n, c) in enumerate(inst):
        if plain[0][i] == 1:
            assert np.array_equal(hinted['own'][1][i], plain[1][i])
            assert hinted['own'][2][i] == exact_model.check_reads(c, plain[1][i])[0] <= plain[2][i]


def test_all_nan_hints_are_the_unhinted_search(batch):
    "P4"
    inst, plain, _, _ = batch
    for hints in (None, [np.full(n, np.nan, dtype=np.float32) for n, _ in inst]):
        got = exact_model.solve(inst, hints)
        np.testing.assert_array_equal(got[0], plain[0])
        np.testing.assert_array_equal(got[2], plain[2])
        assert all(np.array_equal(a, b) for a, b in zip(got[1], plain[1]))


def test_budget_in_the_model():
    rng = np.random.RandomState(6)
    inst = [random_instance(rng, 12) for _ in range(150)]
    hints = [rng.randint(0, 2, size=n).astype(np.float32) for n, _ in inst]
    full = exact_model.solve(inst, hints)
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    for budget in (50, 400):
        s, _, w = exact_model.solve(inst, hints, budget)
        und = s == -1
        assert und.any() and (~und).any()
        assert (w < budget + 3 * edges).all() and (w[und] >= budget).all()
        np.testing.assert_array_equal(s[~und], full[0][~und])
        np.testing.assert_array_equal(w[~und], full[2][~und])
    # the check pass runs before the first budget check
    assert exact_model.search(2, [[1, 2], [-1, 2]], [0.0, 1.0], budget=1)[0] == 1
    assert exact_model.search(2, [[1, 2], [-1, 2]], [1.0, 0.0], budget=1)[0] == -1


def test_hint_wrapper_arguments():
    "native.Problem.exact_solve / exact.solve_items take hints; the symbol is exported"
    import inspect
    from pdp import exact, native
    assert 'pdp_exact_solve_hinted' in native.EXPORTED_SYMBOLS
    assert 'hints' in inspect.signature(native.Problem.exact_solve).parameters
    assert 'hints' in inspect.signature(exact.solve_items).parameters
