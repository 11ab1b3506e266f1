"""The split counting search (pdp_exact_count_split, include/pdp_hip.h) stated in plain Python: one instance's model count from 2^depth cubes.

A cube is tests/exact_count_model.py's search with the decisions of levels 1..depth pinned by the bits of the cube's index, exactly as in
tests/exact_split_model.py (the most significant of the ``depth`` bits belongs to level 1; 0 = the polarity the search tries first, 1 = the
other one; a pinned level counts as already flipped, so backtracking pops through it).  The cubes partition the plain search's tree, so
their counts add.  One more rule makes that true where the tree is shallower than the prefix: a leaf met with fewer than ``depth`` levels
open is reached by every cube that shares those levels' bits, and is credited to the one whose remaining bits are all 0.
All the arithmetic is IEEE double in exactly the order written here -- per cube as in exact_count_model.py, then over the cubes in
ascending index -- and csrc/pdp_exact.hip does the same operations in the same order.  Slow: every cube replays its prefix; meant for
instances of up to about 30 variables."""
import math

import numpy as np

from exact_model import NO_BUDGET

MAX_N = 1023            # as exact_count_model.MAX_N
MAX_DEPTH = 16


def cube(n, clauses, budget, depth, index):
    """(status 1 / -1, count float, true_count float64 [n], work, leaves) of cube ``index`` of the 2^depth cubes.  The budget is the
    cube's own: ``work >= budget`` before every pass, on the cube's own reads."""
    if budget <= 0:
        budget = 1 << 32
    assert 0 <= depth <= MAX_DEPTH and 0 <= index < (1 << depth)
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    assert n <= MAX_N
    work, leaves, count = 0, 0, 0.0
    T, F = [0.0] * n, [0.0] * n
    snap = {0: 0.0}
    val = [0] * n
    trail, mark, dvar = [], {0: 0}, {}
    level = 0

    def credit(lv):
        "the models counted since level lv was opened go to the variables on its part of the trail"
        d = count - snap[lv]
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
        for v in sorted(pend):
            val[v] = 1 if pend[v] & 1 else 2
            conflict = conflict or pend[v] == 3
            trail.append(v)
        if not conflict and pend:
            continue
        if not conflict and wmin is None:
            # a leaf.  Inside the prefix (level < depth) every cube with these levels' bits arrives here: the one whose remaining bits
            # are 0 takes it, the others add nothing; either way the search backtracks as after a conflict
            if level >= depth or index & ((1 << (depth - level)) - 1) == 0:
                count = count + math.ldexp(1.0, n - len(trail))
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
                    snap[level] = count
                    resumed = True
                    break
                level -= 1
            if not resumed:
                break
            continue
        # branching: the unassigned variable with the most occurrences in the open clauses of minimum width, ties to the lower index
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
        positive = cnt.get((v, 1), 0) >= cnt.get((v, 2), 0)
        level += 1
        pinned = level <= depth
        if pinned and (index >> (depth - level)) & 1:                             # the cube's bit of this level: the other polarity
            positive = not positive
        mark[level] = len(trail)
        dvar[level] = (v, pinned)                                                 # a pinned level is never flipped
        snap[level] = count
        val[v] = 1 if positive else 2
        trail.append(v)
    # the end (out of levels, or out of budget): every open level is flushed, the newest first, level 0 with mark 0
    while level >= 0:
        credit(level)
        del trail[mark[level]:]
        level -= 1
    true_count = np.asarray([T[v] + (count - T[v] - F[v]) * 0.5 for v in range(n)], dtype=np.float64)
    return status, count, true_count, work, leaves


def search(n, clauses, budget=NO_BUDGET, depth=0):
    """(status, count, true_count float64 [n], work, leaves, cubes) of the instance from its 2^depth cubes, summed in ascending index:
    status 1 if every cube's is 1, else -1 (count is then a lower bound); cubes = [(status, count, work, leaves)].  n > 1023: status -2,
    every other output 0 and the one record (-2, 0.0, 0, 0), at every depth."""
    cl = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in cl for l in c])
    if n > MAX_N:
        return -2, 0.0, np.zeros(n, dtype=np.float64), 0, 0, [(-2, 0.0, 0, 0)]
    count, work, leaves = 0.0, 0, 0
    true_count = np.zeros(n, dtype=np.float64)
    cubes = []
    for j in range(1 << depth):
        st, c, tc, w, lv = cube(n, cl, budget, depth, j)
        cubes.append((st, c, w, lv))
        count = count + c
        for v in range(n):
            true_count[v] = true_count[v] + tc[v]
        work += w
        leaves += lv
    status = 1 if all(c[0] == 1 for c in cubes) else -1
    return status, count, true_count, work, leaves, cubes


def solve(instances, budget=NO_BUDGET, depths=0):
    "search() over a list (depths: an int or one per instance): a list of its tuples"
    if isinstance(depths, int):
        depths = [depths] * len(instances)
    return [search(n, c, budget, d) for (n, c), d in zip(instances, depths)]
