"""Instances, weights and references shared by test_exact_mass_host.py and test_exact_mass_gpu.py (pdp_exact_mass).  Every cached result
is computed once per process and must not be modified by a test."""
import functools
from fractions import Fraction

import numpy as np

import exact_count_cases as cs
import exact_mass_model as zm
import exact_model

EIGHTHS_SEED = 8          # the draw of small(): 0 < share of mass 0 and of mass > 0, each at least a quarter (asserted by the host test)
SCALE = 149               # every float32 is an integer multiple of 2^-149


def half(n):
    return np.full(n, 0.5, dtype=np.float32)


def eighths(rng, n):
    "multiples of 1/8, 0 and 1 included: every product of at most 10 of them has at most 30 mantissa bits"
    return (rng.randint(0, 9, size=n) / 8.0).astype(np.float32)


def random32(rng, n):
    "float32 values of [0, 1), an exact 0 or 1 now and then"
    w = rng.rand(n).astype(np.float32)
    w[rng.rand(n) < 0.04] = 0.0
    w[rng.rand(n) < 0.04] = 1.0
    return w


def around(model, confidence):
    "``confidence`` on the model's side of every variable, in float32"
    c = np.float32(confidence)
    return np.where(np.asarray(model) > 0.5, c, np.float32(1.0) - c).astype(np.float32)


def size(inst):
    n, clauses = inst
    return max([n] + [abs(int(l)) for c in clauses for l in c])


def brute(n, clauses, weights):
    """(Z, true[n]) as Fractions over all 2^n assignments: exact rational arithmetic on the float32 weights (integers over 2^-149)"""
    rows = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in rows for l in c])
    w32 = np.asarray(weights, dtype=np.float32)
    assert w32.size == n and n <= 12
    grid = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool)
    ok = np.ones(1 << n, dtype=bool)
    for c in rows:
        idx, pos = np.array([abs(l) - 1 for l in c], dtype=np.int64), np.array([l > 0 for l in c])
        ok &= (grid[:, idx] == pos).any(axis=1) if c else False
    one = 1 << SCALE
    prod = np.array([1], dtype=object)
    for v in range(n):                                                                   # bit v of the index is x_v, as in grid
        f = Fraction(float(w32[v])) * one
        assert f.denominator == 1
        a = int(f)
        prod = np.concatenate([prod * (one - a), prod * a])
    den = 1 << (SCALE * n)
    z = Fraction(int(prod[ok].sum()) if ok.any() else 0, den)
    true = [Fraction(int(prod[ok & grid[:, v]].sum()) if (ok & grid[:, v]).any() else 0, den) for v in range(n)]
    return z, true


@functools.lru_cache(maxsize=None)
def small():
    "the instances of exact_count_cases.family() with n <= 10, and their 1/8 weights"
    inst = [i for i in cs.family() if size(i) <= 10]
    rng = np.random.RandomState(EIGHTHS_SEED)
    return inst, [eighths(rng, size(i)) for i in inst]


@functools.lru_cache(maxsize=None)
def small_brute():
    inst, w = small()
    return [brute(n, c, x) for (n, c), x in zip(inst, w)]


@functools.lru_cache(maxsize=None)
def small_random():
    "random float32 weights for small()'s instances"
    rng = np.random.RandomState(3232)
    return [random32(rng, size(i)) for i in small()[0]]


@functools.lru_cache(maxsize=None)
def family_weights(kind):
    "weights of one kind ('half', 'eighths', 'random') for every instance of exact_count_cases.family()"
    rng = np.random.RandomState({'half': 1, 'eighths': 88, 'random': 323}[kind])
    make = {'half': lambda n: half(n), 'eighths': lambda n: eighths(rng, n), 'random': lambda n: random32(rng, n)}[kind]
    return [make(size(i)) for i in cs.family()]


def satisfiable_3sat(seed, n, ratios, each):
    "uniform 3-SAT instances that have a model, with the deciding model's one: [((n, clauses), model)]"
    rng = np.random.RandomState(seed)
    out = []
    for r in ratios:
        got = 0
        while got < each:
            inst = cs.threshold_3sat(rng, n, int(round(r * n)))
            st, model, _ = exact_model.search(*inst)
            if st == 1:
                out.append((inst, np.asarray(model, dtype=np.float32)))
                got += 1
    return out


def same(a, b):
    "two results in the layout of exact_mass_model.solve: equal bit for bit, with equal dtypes"
    for i in (0, 1, 3, 4, 5):
        np.testing.assert_array_equal(a[i], b[i])
        assert a[i].dtype == b[i].dtype, (i, a[i].dtype, b[i].dtype)
    assert len(a[2]) == len(b[2])
    for p, q in zip(a[2], b[2]):
        assert p.dtype == q.dtype == np.float64
        np.testing.assert_array_equal(p, q)


def pick(res, idx):
    return tuple([res[k][i] for i in idx] if k == 2 else res[k][idx] for k in range(6))


def join(a, b):
    return tuple(x + y if k == 2 else np.concatenate([x, y]) for k, (x, y) in enumerate(zip(a, b)))


def exact(x):
    return Fraction(float(x))


def check_bracket(n, got, z_full, leaves_full):
    """mass <= Z_full <= mass + open_mass, compared exactly as Fractions of the doubles; the model's rounding bound (of the complete run)
    is allowed on the right-hand side only"""
    st, mass, _, open_mass = got[:4]
    assert exact(mass) <= exact(z_full), (mass, z_full)
    slack = exact(zm.mass_bound(n, leaves_full, z_full))
    assert exact(z_full) <= exact(mass) + exact(open_mass) + slack, (mass, open_mass, z_full)
