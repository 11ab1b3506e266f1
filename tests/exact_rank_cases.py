"""Instances and helpers shared by test_exact_rank_host.py and test_exact_rank_gpu.py (pdp_exact_models_at)."""
import functools

import numpy as np

import exact_count_cases as cs
import exact_count_model as cm

TOP = (1 << 53) - 1          # the largest rank


def brute_models(n, clauses):
    "the models of the instance over all 2^n assignments as a set of byte strings (one 0/1 byte per variable)"
    rows = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in rows for l in c])
    grid = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)
    return {r.tobytes() for r in grid[satisfied(grid, rows)]}


def satisfied(models, clauses):
    "boolean [K]: row k of models (0/1 [K, n]) satisfies every clause"
    m = np.asarray(models).astype(bool)
    ok = np.ones(m.shape[0], dtype=bool)
    for c in clauses:
        c = [int(l) for l in c if int(l) != 0]
        idx, pos = np.array([abs(l) - 1 for l in c], dtype=np.int64), np.array([l > 0 for l in c], dtype=bool)
        ok &= (m[:, idx] == pos).any(axis=1) if c else False
    return ok


def bits(r, k):
    "the k lowest binary digits of r, lowest first"
    return [(int(r) >> j) & 1 for j in range(k)]


def fixed_prefix():
    "n = 110: unit clauses fix variables 1 .. 70 (alternating), 71 .. 110 are free: one leaf of 2^40 models; the free block starts inside the second chunk of 64"
    return 110, [[v if v % 2 else -v] for v in range(1, 71)]


def fixed_evens():
    "n = 130: every even variable is fixed true, the 65 odd ones are free: one leaf of 2^65 models, free variables in all three chunks"
    return 130, [[v] for v in range(2, 131, 2)]


PATTERNS = sorted({0, 1, 5, (1 << 40) - 1, 1 << 39, 0x5555555555 & ((1 << 40) - 1), 0xAAAAAAAAAA & ((1 << 40) - 1), (1 << 23) | (1 << 24) | 1})
WIDE_RANKS = sorted({0, 1, 1 << 22, 1 << 23, (1 << 32) - 1, 1 << 52, TOP - 1, TOP})


@functools.lru_cache(maxsize=None)
def family_counts():
    "exact_count_model.search of every instance of exact_count_cases.family()"
    return [cm.search(n, c) for n, c in cs.family()]


def family_ranks():
    "for every instance of the family: all its ranks and one beyond"
    return [list(range(int(r[1]) + 1)) for r in family_counts()]


def same(a, b):
    "two results in the layout of exact_rank_model.solve: equal bit for bit, with equal dtypes and shapes"
    for i in (0, 1, 4, 5):
        np.testing.assert_array_equal(a[i], b[i])
        assert a[i].dtype == b[i].dtype, (i, a[i].dtype, b[i].dtype)
    for i, dt in ((2, np.int8), (3, np.uint8)):
        assert len(a[i]) == len(b[i])
        for p, q in zip(a[i], b[i]):
            assert p.dtype == q.dtype == dt and p.shape == q.shape, (i, p.dtype, q.dtype, p.shape, q.shape)
            np.testing.assert_array_equal(p, q)


def pick(res, idx):
    return tuple([res[k][i] for i in idx] if k in (2, 3) else res[k][idx] for k in range(6))
