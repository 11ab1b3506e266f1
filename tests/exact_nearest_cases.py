"""Instances, hints, penalties and references shared by test_exact_nearest_host.py, test_exact_nearest_gpu.py and
test_exact_nearest_reuse_gpu.py (pdp_exact_nearest).  Every result is computed once per process (functools.lru_cache) and must not be
modified by a test."""
import functools

import numpy as np

import exact_count_cases as cc
import exact_model
import exact_nearest_model as nm

CAP = nm.MAX_PENALTY
MIXED = (0, 1, 2, 7, CAP)
HINT_KINDS = ('random', 'false', 'model', 'flips')


def brute(n, clauses, bits, pen):
    "(the least penalty distance from ``bits`` over the models of the instance, or None without a model; the models as a bool grid)"
    rows = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in rows for l in c])
    grid = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    ok = np.ones(1 << n, dtype=bool)
    for c in rows:
        idx, pos = np.array([abs(l) - 1 for l in c], dtype=np.int64), np.array([l > 0 for l in c])
        ok &= (grid[:, idx] == pos).any(axis=1) if c else False
    models = grid[ok]
    if not len(models):
        return None, models
    cost = ((models != np.asarray(bits, dtype=bool)[None, :]) * np.asarray(pen, dtype=np.int64)[None, :]).sum(axis=1)
    return int(cost.min()), models


def satisfies(clauses, model):
    return all(any((model[abs(int(l)) - 1] > 0.5) == (int(l) > 0) for l in c if int(l) != 0) for c in clauses)


def any_model(n, clauses):
    "a model by the plain deciding search's statement, or None"
    st, model, _ = exact_model.search(n, clauses)
    return model if st == 1 else None


def hint_of(rng, n, clauses, kind):
    "random 0/1; None (all false); a model (random where there is none); a model with 1 .. 5 flips"
    if kind == 'false':
        return None
    h = rng.randint(0, 2, size=n).astype(np.float32)
    if kind in ('model', 'flips'):
        m = any_model(n, clauses)
        if m is not None:
            h = m.copy()
            if kind == 'flips':
                at = rng.choice(n, size=min(n, int(rng.randint(1, 6))), replace=False)
                h[at] = 1.0 - h[at]
    return h


def penalties_of(rng, n):
    return rng.choice(MIXED, size=n, p=[0.15, 0.35, 0.25, 0.2, 0.05]).astype(np.int32)


def dress(inst, seed):
    "per instance a hint (the kinds in turn) and mixed penalties"
    rng = np.random.RandomState(seed)
    hints = [hint_of(rng, n, c, HINT_KINDS[i % len(HINT_KINDS)]) for i, (n, c) in enumerate(inst)]
    return hints, [penalties_of(rng, n) for n, _ in inst]


@functools.lru_cache(maxsize=None)
def small():
    "the brute-force family of the count (n <= 12: clause widths 0 to 4, repeated literals, tautologies, empty clauses, unused variables, families.py)"
    inst = list(cc.family())
    hints, pens = dress(inst, 4100)
    return inst, hints, pens


UNIFORM_N, UNIFORM_RATIOS = (20, 30, 50), (3.5, 4.0, 4.5)
UNIFORM_EACH = {20: 6, 30: 4, 50: 2}
READ_LIMIT = 1 << 22


@functools.lru_cache(maxsize=None)
def uniform():
    "uniform 3-SAT n = 20 / 30 / 50 at ratios 3.5 / 4.0 / 4.5; the hint kinds in turn, mixed penalties"
    inst = []
    for n in UNIFORM_N:
        inst += cc.uniform_3sat(5200 + n, n, UNIFORM_RATIOS, UNIFORM_EACH[n])
    hints, pens = dress(inst, 4200)
    return inst, hints, pens


@functools.lru_cache(maxsize=None)
def batch():
    "one problem of a few hundred instances: small() and uniform()"
    a, b = small(), uniform()
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


@functools.lru_cache(maxsize=None)
def results(mixed, budget=nm.NO_BUDGET):
    "the model on batch(), with the mixed penalties or with none"
    inst, hints, pens = batch()
    return nm.solve(inst, hints, pens if mixed else None, budget)


def fan_case(k=150):
    "{(x1 | y_i)}, the hint false on every y_i and on x1, x1 heavy: the first model is x1 false with k units against the hint on one level"
    n, clauses = cc.fan(k)
    pen = np.ones(n, dtype=np.int32)
    pen[0] = k + 5
    return (n, clauses), np.zeros(n, dtype=np.float32), pen


def units_case(n=4100):
    "n unit clauses (x_i), hint all false, penalty 2^20 each: one pass, 65 chunks, cost n * 2^20 > 2^32"
    return (n, [[i + 1] for i in range(n)]), np.zeros(n, dtype=np.float32), np.full(n, CAP, dtype=np.int32)


def fill_case(extra=100):
    "a satisfiable 12-variable core and ``extra`` unused variables whose hint is true; the core's hint is the complement of a model"
    (n, clauses), _ = cc.padded_core(extra)
    m = any_model(12, clauses)
    hint = np.ones(n, dtype=np.float32)
    hint[:12] = 1.0 - m
    return (n, clauses), hint, np.ones(n, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def wide_batch():
    "the instances of tests/exact_wide.py that put trails past 128, with random hints and mixed penalties"
    import exact_wide as xw
    inst = [(n, cl) for n, (_, cl) in zip(xw.sizes(xw.plain_batch()), xw.plain_batch())]
    rng = np.random.RandomState(4300)
    hints = [rng.randint(0, 2, size=n).astype(np.float32) for n, _ in inst]
    return inst, hints, [penalties_of(rng, n) for n, _ in inst]


WIDE_BUDGET = 300_000


@functools.lru_cache(maxsize=None)
def wide_results():
    inst, hints, pens = wide_batch()
    stats = [{} for _ in inst]
    out = [nm.search(n, c, hints[i], pens[i], WIDE_BUDGET, stats=stats[i]) for i, (n, c) in enumerate(inst)]
    return pack(out), stats


def pack(out):
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.int64), [o[2] for o in out],
            np.array([o[3] for o in out], dtype=np.int64), np.array([o[4] for o in out], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def slab_case():
    "section 9.8's instance of the HBM route (n = 10, 3 000 clauses of 8 literals around planted models), a random hint, mixed penalties"
    n, clauses = cc.past_the_slab()
    rng = np.random.RandomState(4400)
    return (n, clauses), rng.randint(0, 2, size=n).astype(np.float32), np.array([7, 1, 2, 1, 0, 7, 1, 2, 1, 1], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def slab_result():
    inst, hint, pen = slab_case()
    return nm.search(*inst, hint, pen)


def edges(inst):
    return np.array([sum(len([l for l in c if int(l) != 0]) for c in cl) for _, cl in inst], dtype=np.int64)


def same(a, b):
    "two results in the layout of exact_nearest_model.solve: equal in all five outputs, with equal dtypes"
    for i in (0, 1, 3, 4):
        np.testing.assert_array_equal(a[i], b[i])
        assert a[i].dtype == b[i].dtype, (i, a[i].dtype, b[i].dtype)
    assert len(a[2]) == len(b[2])
    for p, q in zip(a[2], b[2]):
        np.testing.assert_array_equal(p, q)


def pick(res, idx):
    return tuple([res[k][i] for i in idx] if k == 2 else res[k][idx] for k in range(5))
