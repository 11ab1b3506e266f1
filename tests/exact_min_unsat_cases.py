"""Instances, hints and references shared by test_exact_min_unsat_host.py and test_exact_min_unsat_gpu.py (pdp_exact_min_unsat)."""
import functools
import itertools

import numpy as np

import exact_min_unsat_model as mm
from test_exact_gpu import DEGENERATE, random_instance

KINDS = ('random', 'nan30', 'none')
LDS_LIMIT = 48 * 1024


def brute_min(n, clauses):
    "the minimum number of unsatisfied clauses over all assignments of the variables that occur (the others change nothing)"
    rows = [[int(l) for l in c if int(l) != 0] for c in clauses]
    used = sorted({abs(l) for c in rows for l in c})
    at = {v: i for i, v in enumerate(used)}
    want = [(np.array([at[abs(l)] for l in c], dtype=np.int64), np.array([l > 0 for l in c])) for c in rows]
    if not used:
        return len(rows)
    grid = np.array(list(itertools.product((False, True), repeat=len(used))), dtype=bool)
    cost = np.zeros(len(grid), dtype=np.int64)
    for idx, pos in want:
        cost += ~(grid[:, idx] == pos).any(axis=1) if len(idx) else 1
    return int(cost.min())


def hints_of(rng, inst, kind):
    "per instance: random 0/1, uniform values with 30 % NaN, or None"
    out = []
    for n, _ in inst:
        if kind == 'none':
            out.append(None)
            continue
        h = rng.randint(0, 2, size=n).astype(np.float32) if kind == 'random' else rng.rand(n).astype(np.float32)
        if kind == 'nan30':
            h[rng.rand(n) < 0.3] = np.nan
        out.append(h)
    return out


def family(seed, count, n_max):
    "count instances of random_instance(rng, n_max) plus DEGENERATE, and the three kinds of hints for them"
    rng = np.random.RandomState(seed)
    inst = [random_instance(rng, n_max) for _ in range(count)] + DEGENERATE
    return inst, {k: hints_of(rng, inst, k) for k in KINDS}


def threshold_3sat(rng, n, m):
    clauses = []
    for _ in range(m):
        vs = rng.choice(n, size=3, replace=False) + 1
        clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
    return n, clauses


def block(a, b, c):
    "the eight sign patterns over three variables: every assignment falsifies exactly one of them"
    return [[sa * a, sb * b, sc * c] for sa in (1, -1) for sb in (1, -1) for sc in (1, -1)]


CHAIN = 4


def wide(F):
    """(n, clauses), hint: an instance with n = 11 + 2 F variables and 21 + 3 F clauses whose optimum is 2 -- two blocks over fresh
    variables, everything else satisfiable -- and a hint that leaves 3 clauses unsatisfied.
      x = 1               the unit clause [x]; hinted true
      e_1 .. e_4          the chain [e_1], e_1 -> e_2, ..., hinted true but for e_4: the hint's third unsatisfied clause
      y_i, z_i (F each)   padding that x satisfies: (x | y_i), (x | z_i), (x | -y_i | -z_i)
      a_1..3, b_1..3      the two blocks
    The search decides x on its width-1 clause, walks the chain by decisions (cost 0 < ub - 1: nothing is forced), meets cost 3 under
    e_4 = false, flips it and finds the leaf of cost 2: an improvement.  With ub = 2 every flipped decision costs 1 and forces: under
    x = false one pass forces the 2 F variables y_i, z_i (a trail of 2 F + 1), and the next one finds F clauses falsified."""
    x, e = 1, list(range(2, 2 + CHAIN))
    y = list(range(2 + CHAIN, 2 + CHAIN + F))
    z = list(range(2 + CHAIN + F, 2 + CHAIN + 2 * F))
    a = list(range(2 + CHAIN + 2 * F, 8 + CHAIN + 2 * F))
    clauses = [[x], [e[0]]] + [[-e[i], e[i + 1]] for i in range(CHAIN - 1)]
    for yi, zi in zip(y, z):
        clauses += [[x, yi], [x, zi], [x, -yi, -zi]]
    clauses += block(*a[:3]) + block(*a[3:])
    n = a[-1]
    hint = np.zeros(n, dtype=np.float32)
    hint[[x - 1] + [v - 1 for v in e[:-1]] + [v - 1 for v in y]] = 1.0
    return (n, clauses), hint


WIDE_F = (70, 100)


def slab_bytes(n, m, e):
    "csrc/pdp_exact.hip ex_lds_layout"
    return (25 * n + 8 + 2 * e + 2 * (m + 1) + 15) & ~15


def past_the_slab():
    """An instance of the HBM route that brute force can still answer: 10 variables, 3 000 random clauses of 8 distinct ones each.  The
    24 000 literals take the slab past 48 KiB; there are at most 1 024 leaves (the model needs about two seconds).  An assignment
    falsifies 3000 / 256 clauses on average, the best one 2; the hint is random."""
    rng = np.random.RandomState(91)
    n, m = 10, 3000
    clauses = []
    for _ in range(m):
        vs = rng.choice(n, size=8, replace=False) + 1
        clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=8))])
    assert slab_bytes(n, m, 8 * m) > LDS_LIMIT
    return (n, clauses), rng.randint(0, 2, size=n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide_results(F):
    "the model's five outputs and its stats on wide(F)"
    inst, hint = wide(F)
    stats = {}
    return mm.search(*inst, hint, stats=stats), stats


@functools.lru_cache(maxsize=None)
def slab_result():
    inst, hint = past_the_slab()
    return mm.search(*inst, hint)
