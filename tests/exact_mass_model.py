"""The weighted counting search (pdp_exact_mass, include/pdp_hip.h) stated in plain Python: status, mass, true_mass, open_mass, work and
leaves of one instance under a product prior, Z(p) = sum over the models x of prod_v (p_v if x_v else 1 - p_v).

tests/exact_count_model.py's search with weights: the positive literal of v weighs p_v = double(float32 weight), the negative one
1.0 - p_v (computed in double wherever it is used), an unassigned variable nothing.  ``mass`` is the product of the weights of everything
on the trail, ``pre[level]`` its value before the level's decision, a leaf adds ``mass`` to Z, and the first polarity of a decision is
the heavier literal (at exactly 0.5 the count's rule).  A state whose mass is 0.0 is a conflict: after a pass, and at once where a flip
multiplies by a weight of 0.  When the budget fires, the mass of the
part of the tree not yet visited is summed from ``pre`` (open_mass).  Every double operation stands here in the order csrc/pdp_exact.hip
performs it -- add, subtract and multiply only -- so the GPU results are compared with array_equal.

The error of this order against exact arithmetic, to first order in u = 2^-53 (tests: BOUND_FACTOR = 2 for the second-order terms):
  * 1.0 - p_v is exact for a float32 p_v in [0, 1] held in a double (p_v is a multiple of 2^-149 with 24 significant bits; for
    p_v >= 2^-29 the difference needs at most 53 bits, below that it rounds with relative error u -- counted with the products);
  * the mass at a leaf is a product of at most n factors, each multiplication rounds once: relative error at most n u (the butterfly
    and the chunk order change which partial products exist, not how many roundings lie on the path from a factor to the result:
    at most 6 + chunks + levels <= n + 6 of them; the bound below uses n + 6);
  * Z is a sequential sum of ``leaves`` non-negative terms: |Z - Z*| <= (n + 6 + leaves) u Z*            (mass_bound)
  * T[v] and F[v] are sums of at most 2 leaves + 2 credits (every undone level that held v: a level is undone at most twice per leaf
    below it, plus the end flush), each credit the difference of two partial sums of Z, each of absolute error at most
    (n + 6 + leaves) u Z*, and each addition rounds once more on a value <= Z*; true_mass adds one subtraction pair and one product:
    |true_mass[v] - exact| <= 2 (leaves + 1) (n + 6 + leaves) u Z* + (2 leaves + 6) u Z*                 (true_mass_bound)
Slow: meant for small instances."""
import numpy as np

from exact_model import NO_BUDGET

MAX_N = 1023            # as the count: a larger instance gets status -2, so the slab extension stays bounded
U = 2.0 ** -53
BOUND_FACTOR = 2.0


def mass_bound(n, leaves, z):
    "|mass - Z*| of a complete run, from the operation order (docstring), with the factor for the second-order terms"
    return BOUND_FACTOR * (n + 6 + leaves) * U * z


def true_mass_bound(n, leaves, z):
    "|true_mass[v] - exact| of a complete run, from the operation order (docstring), with the factor for the second-order terms"
    return BOUND_FACTOR * (2 * (leaves + 1) * (n + 6 + leaves) + 2 * leaves + 6) * U * z


def chunk_product(factors):
    "the product of at most 64 doubles as the wave forms it: lanes without a factor hold 1.0, xor butterfly 32, 16, 8, 4, 2, 1"
    x = np.ones(64, dtype=np.float64)
    x[:len(factors)] = factors
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x * x[lanes ^ o]
    return float(x[0])


def search(n, clauses, weights, budget=NO_BUDGET, *, prune=True):
    """(status 1 / -1 / -2 / -3, mass float, true_mass float64 [n], open_mass float, work, leaves) of the instance (n, clauses: lists of
    signed 1-based ints) under ``weights`` (n values, taken as float32).  status 1: mass is Z and true_mass[v] the part of it with v
    true; -1: the budget ran out, both cover the part of the tree visited so far and Z lies in [mass, mass + open_mass]; -2: n > 1023;
    -3: a weight is NaN or outside [0, 1]; neither is searched and every other output is 0.  ``prune=False`` (tests only) switches the
    zero-mass rule off."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    w32 = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert w32.size == n, (w32.size, n)
    if n > MAX_N:
        return -2, 0.0, np.zeros(n, dtype=np.float64), 0.0, 0, 0
    if not bool(((w32 >= 0) & (w32 <= 1)).all()):                                 # a NaN fails both comparisons
        return -3, 0.0, np.zeros(n, dtype=np.float64), 0.0, 0, 0
    p = [float(x) for x in w32]

    def omega(v, x):
        return p[v] if x == 1 else 1.0 - p[v]

    work, leaves, Z, mass = 0, 0, 0.0, 1.0
    T, F = [0.0] * n, [0.0] * n
    snap, pre = {0: 0.0}, {}
    val = [0] * n
    trail, mark, dvar = [], {0: 0}, {}
    level = 0

    def credit(lv):
        "the mass counted since level lv was opened goes to the variables on its part of the trail"
        d = Z - snap[lv]
        for u in trail[mark[lv]:]:
            if val[u] == 1:
                T[u] += d
            else:
                F[u] += d

    status = 1
    while True:
        if work >= budget:
            status = -1
            break
        # one unit-propagation pass
        conflict, pend, wmin = False, {}, None
        for c in cls:
            nfree, sat, first, distinct, k = 0, False, None, False, 0
            for L in c:
                k += 1
                x = val[L[0]]
                if x == 0:
                    if nfree == 0:
                        first = L
                    elif L != first:
                        distinct = True
                    nfree += 1
                elif x == L[1]:
                    sat = True
                    break
            work += k
            if sat:
                continue
            if nfree == 0:
                conflict = True
            elif not distinct:
                pend[first[0]] = pend.get(first[0], 0) | first[1]
            else:
                wmin = nfree if wmin is None else min(wmin, nfree)
        old = len(trail)
        for v in sorted(pend):
            val[v] = 1 if pend[v] & 1 else 2
            conflict = conflict or pend[v] == 3
            trail.append(v)
        # the pass's new entries, 64 consecutive ones at a time, ascending
        for base in range(old, len(trail), 64):
            mass = mass * chunk_product([omega(u, val[u]) for u in trail[base:base + 64]])
        if prune and mass == 0.0:
            conflict = True
        if not conflict and pend:
            continue
        if not conflict and wmin is None:
            # a leaf: every clause has a true literal, the unassigned variables are free and contribute a factor 1
            Z = Z + mass
            leaves += 1
            conflict = True
        if conflict:
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
                credit(level)
                for u in trail[mark[level]:]:
                    val[u] = 0
                del trail[mark[level]:]
                if not second:
                    dvar[level] = (v, True)
                    val[v] = 3 - first
                    trail.append(v)
                    snap[level] = Z
                    mass = pre[level] * omega(v, val[v])
                    if prune and mass == 0.0:
                        continue        # the other half has no mass: a conflict at once, without a pass (the level is undone next)
                    resumed = True
                    break
                level -= 1
            if not resumed:
                break
            continue
        # branching: the count's variable; the heavier literal first, the count's polarity at exactly 0.5
        cnt = {}
        for c in cls:
            nfree, sat, k = 0, False, 0
            for L in c:
                k += 1
                x = val[L[0]]
                if x == 0:
                    nfree += 1
                elif x == L[1]:
                    sat = True
                    break
            work += k
            if sat or nfree != wmin:
                continue
            for L in c:
                if val[L[0]] == 0:
                    cnt[L] = cnt.get(L, 0) + 1
            work += len(c)
        score = {}
        for (v, _), k in cnt.items():
            score[v] = score.get(v, 0) + k
        v = max(score, key=lambda u: (score[u], -u))
        if p[v] > 0.5:
            positive = True
        elif p[v] < 0.5:
            positive = False
        else:
            positive = cnt.get((v, 1), 0) >= cnt.get((v, 2), 0)
        level += 1
        mark[level] = len(trail)
        dvar[level] = (v, False)
        pre[level] = mass
        snap[level] = Z
        val[v] = 1 if positive else 2
        trail.append(v)
        mass = mass * omega(v, val[v])
    # the mass not yet visited: the untried halves of the open levels, oldest first, then the current node (the budget check fires
    # before a pass, so it is unresolved)
    open_mass = 0.0
    if status == -1:
        for lv in range(1, level + 1):
            v, second = dvar[lv]
            if not second:
                open_mass = open_mass + pre[lv] * omega(v, 3 - val[v])
        open_mass = open_mass + mass
    # the end (out of levels, or out of budget): every open level is flushed, the newest first, level 0 with mark 0
    while level >= 0:
        credit(level)
        del trail[mark[level]:]
        level -= 1
    true_mass = np.asarray([T[v] + (Z - T[v] - F[v]) * p[v] for v in range(n)], dtype=np.float64)
    return status, Z, true_mass, open_mass, work, leaves


def solve(instances, weights, budget=NO_BUDGET):
    """search() over a list: (status int8 [N], mass float64 [N], true_masses list, open_mass float64 [N], work int64 [N],
    leaves int64 [N])"""
    out = [search(n, c, w, budget) for (n, c), w in zip(instances, weights)]
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.float64), [o[2] for o in out],
            np.array([o[3] for o in out], dtype=np.float64), np.array([o[4] for o in out], dtype=np.int64),
            np.array([o[5] for o in out], dtype=np.int64))
