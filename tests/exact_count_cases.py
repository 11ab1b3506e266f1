"""Instances and references shared by test_exact_count_host.py and test_exact_count_gpu.py (pdp_exact_count)."""
import functools

import numpy as np

import exact_count_model as cm
import families
from exact_min_unsat_cases import LDS_LIMIT, slab_bytes, threshold_3sat

DEGENERATE = [
    (4, []),                                      # no clauses: 16 models
    (3, [[2]]),                                   # a unit clause, two variables without occurrences
    (2, [[1], [-1]]),                             # contradicting units: 0 models
    (2, [[1, 1, 1], [-1, 2, -1], [-2, -2]]),      # repeated literals: 0 models
    (3, [[1, 1, 2], [-1, -1], [3, 3]]),           # repeated literals: 1 model
    (2, [[1, -1]]),                               # a tautology: 4 models
    (3, [[1, -1, 2], [-2, 2], [-1], [3, -3, -3]]),
    (5, [[1, 2], [], [3]]),                       # an empty clause: 0 models
    (6, [[6], [-6, 5], [-5, 4], [-4, 3], [-3, 2], [-2, 1]]),
    (7, [[1, 2], [3, 4]]),                        # three unused variables
]


def random_instance(rng, n_max=12):
    """n <= n_max variables, of which the last few may be unused; clauses of 0 to 4 literals drawn WITH replacement over the variables and
    the signs, so repeated literals and tautologies occur; between 0.3 n and 3 n clauses, so most instances have models"""
    n = int(rng.randint(1, n_max + 1))
    used = int(rng.randint(1, n + 1)) if rng.rand() < 0.3 else n
    clauses = []
    for _ in range(int(round(rng.uniform(0.3, 3.0) * n))):
        k = int(rng.choice([0, 1, 2, 3, 4], p=[0.02, 0.08, 0.3, 0.4, 0.2]))
        clauses.append([int(v) * int(s) for v, s in zip(rng.randint(1, used + 1, size=k), rng.choice([-1, 1], size=k))])
    return n, clauses


def from_families():
    "instances of tests/families.py that brute force can answer (n <= 12)"
    R = np.random.RandomState
    out = [(n, c) for n, c in families.minimal(R(13000)) if n <= 12]
    out += [families.unit_chain(L) for L in (1, 5, 12)] + [families.pure_cascade(L) for L in (2, 7, 11)]
    out += [families.ladder(R(31000 + i), 12, a) for i, a in enumerate((2.0, 3.0, 4.26, 4.26, 5.0))]
    out += [families.hub(R(31100 + i), d, n=12, m=20) for i, d in enumerate((4, 9))]
    out += [families.regular(R(31200 + i), 4, 3, 12) for i in range(3)]
    return out


@functools.lru_cache(maxsize=None)
def family(seed=77, count=380):
    "count random instances plus the degenerate ones plus those from families.py, all with n <= 12"
    rng = np.random.RandomState(seed)
    return [random_instance(rng) for _ in range(count)] + DEGENERATE + from_families()


def brute(n, clauses):
    "(count, true_count int64 [n]) over all 2^n assignments, unused variables included"
    rows = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in rows for l in c])
    grid = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    ok = np.ones(1 << n, dtype=bool)
    for c in rows:
        idx, pos = np.array([abs(l) - 1 for l in c], dtype=np.int64), np.array([l > 0 for l in c])
        ok &= (grid[:, idx] == pos).any(axis=1) if c else False
    return int(ok.sum()), grid[ok].sum(axis=0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def family_brute():
    return [brute(n, c) for n, c in family()]


def fan(k):
    "{(x1 | y_i) : i = 1..k}: x1 true leaves every y free (2^k models), x1 false forces all k of them on one level (one model)"
    return k + 1, [[1, i + 2] for i in range(k)]


FAN_K = (60, 150)


def padded_core(extra=60):
    "a satisfiable 12-variable core (3-SAT, 40 clauses) and ``extra`` variables that occur nowhere: (n, clauses), the core's own count"
    rng = np.random.RandomState(12)
    while True:
        n, clauses = threshold_3sat(rng, 12, 40)
        count = brute(n, clauses)[0]
        if count > 0:
            return (n + extra, clauses), count


def past_the_slab():
    """An instance of the HBM route that brute force can still answer: 10 variables, 3 000 random clauses of 8 distinct variables each, kept
    only where every one of 40 planted assignments satisfies them, so the instance has at least that many models (fewer if two plants
    coincide).  The 24 000 literals take the slab past 48 KiB."""
    rng = np.random.RandomState(92)
    n, m = 10, 3000
    plants = rng.randint(0, 2, size=(40, n))
    clauses = []
    while len(clauses) < m:
        vs = rng.choice(n, size=8, replace=False)
        sg = rng.choice([-1, 1], size=8)
        if ((plants[:, vs] == 1) == (sg > 0)).any(axis=1).all():
            clauses.append([int(v + 1) * int(s) for v, s in zip(vs, sg)])
    assert slab_bytes(n, m, 8 * m) > LDS_LIMIT
    return n, clauses


@functools.lru_cache(maxsize=None)
def slab_result():
    return cm.search(*past_the_slab())


def uniform_3sat(seed, n, ratios, each):
    "``each`` instances of uniform 3-SAT on n variables at every clause ratio of ``ratios``"
    rng = np.random.RandomState(seed)
    return [threshold_3sat(rng, n, int(round(r * n))) for r in ratios for _ in range(each)]


def same(a, b):
    "two results in the layout of exact_count_model.solve: equal bit for bit, with equal dtypes"
    for i in (0, 1, 3, 4):
        np.testing.assert_array_equal(a[i], b[i])
        assert a[i].dtype == b[i].dtype, (i, a[i].dtype, b[i].dtype)
    assert len(a[2]) == len(b[2])
    for p, q in zip(a[2], b[2]):
        assert p.dtype == q.dtype == np.float64
        np.testing.assert_array_equal(p, q)


def pick(res, idx):
    return tuple([res[k][i] for i in idx] if k == 2 else res[k][idx] for k in range(5))
