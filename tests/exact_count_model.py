"""The counting complete search (pdp_exact_count, include/pdp_hip.h) stated in plain Python: status, count, true_count, work and leaves
of one instance.

tests/exact_model.py's search without hints, except that a state without an open clause does not end it: the leaf is credited with
2^(unassigned variables) models and the search backtracks as after a conflict.  ``snap[level]`` is the count when a level was opened (or
its decision flipped); when a level is undone, the difference is added to T[u] or F[u] of every variable u on the level's part of the
trail.  All of this arithmetic is IEEE double (Python floats) in exactly the order written here, and csrc/pdp_exact.hip does the same
operations in the same order, so the GPU results can be compared with array_equal even where they round.  It counts the same
clause-literal reads as exact_model.py.  If count <= 2^53 every value is an exact integer.  Slow: meant for small instances."""
import math

import numpy as np

from exact_model import NO_BUDGET, peak

MAX_N = 1023            # 2^n and every partial sum are finite doubles up to here; a larger instance gets status -2


def search(n, clauses, budget=NO_BUDGET, *, stats=None):
    """(status 1 / -1 / -2, count float, true_count float64 [n], work, leaves) of the instance (n, clauses: lists of signed 1-based ints).
    status 1: count is the number of models and true_count[v] the number of them with v true; -1: the budget ran out, both cover the
    part of the tree visited so far; -2: n > 1023, nothing is searched.  ``stats``: a dict that receives the maxima over the run of
    ``trail`` (trail length at a backtrack), ``pass_units`` and ``undone`` (trail entries of one undone level); the results do not
    depend on it."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    if n > MAX_N:
        return -2, 0.0, np.zeros(n, dtype=np.float64), 0, 0
    work, leaves, count = 0, 0, 0.0
    T, F = [0.0] * n, [0.0] * n
    snap = {0: 0.0}
    val = [0] * n
    trail, mark, dvar = [], {0: 0}, {}
    level = 0

    def credit(lv):
        "the models counted since level lv was opened go to the variables on its part of the trail"
        d = count - snap[lv]
        peak(stats, 'undone', len(trail) - mark[lv])
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
        peak(stats, 'pass_units', len(pend))
        if not conflict and pend:
            continue
        if not conflict and wmin is None:
            # a leaf: every clause has a true literal, the unassigned variables are free
            count = count + math.ldexp(1.0, n - len(trail))
            leaves += 1
            conflict = True
        if conflict:
            peak(stats, 'trail', len(trail))
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
        mark[level] = len(trail)
        dvar[level] = (v, False)
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


def solve(instances, budget=NO_BUDGET):
    "search() over a list: (status int8 [N], count float64 [N], true_counts list, work int64 [N], leaves int64 [N])"
    out = [search(n, c, budget) for n, c in instances]
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.float64), [o[2] for o in out],
            np.array([o[3] for o in out], dtype=np.int64), np.array([o[4] for o in out], dtype=np.int64))
