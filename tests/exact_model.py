"""The hinted complete search (pdp_exact_solve_hinted, include/pdp_hip.h) stated in plain Python: status, model and work of one instance.

It follows csrc/pdp_exact.hip pass by pass -- a propagation pass reads every clause up to its first true literal and applies its units at
its end, the branching scan counts the unassigned literals of the open clauses of minimum width, backtracking is chronological -- and counts
the same clause-literal reads, so the GPU results can be compared with array_equal.  Without hints (hints=None, or all NaN) it is
pdp_exact_solve.  Slow: meant for instances of up to about 20 variables."""
import math

import numpy as np

NO_BUDGET = 1 << 62


def hint_codes(n, hints):
    "0 no hint (NaN), 1 true first (h > 0.5), 2 false first (any other finite value)"
    if hints is None:
        return [0] * n
    assert len(hints) == n
    return [0 if math.isnan(float(h)) else (1 if float(h) > 0.5 else 2) for h in hints]


def check_reads(clauses, bits):
    "(reads of the check pass under the 0/1 assignment ``bits``, every clause has a true literal?)"
    reads, ok = 0, True
    for c in clauses:
        k = next((j + 1 for j, l in enumerate(c) if (bits[abs(l) - 1] > 0.5) == (l > 0)), None)
        reads += len(c) if k is None else k
        ok = ok and k is not None
    return reads, ok


def peak(stats, key, value):
    "stats[key] = the maximum seen so far (stats None: nothing is recorded)"
    if stats is not None:
        stats[key] = max(stats.get(key, 0), value)


def search(n, clauses, hints=None, budget=NO_BUDGET, *, stats=None):
    """(status 1 / 0 / -1, model float32 [n], work) of the instance (n, clauses: lists of signed 1-based ints) under ``hints`` ([n] floats or None).
    ``stats``: a dict that receives the maxima over the run of ``trail`` (trail length at a conflict), ``pass_units`` (variables assigned by
    one pass) and ``undone`` (trail entries cleared by one backtrack step); the results do not depend on it."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    code = hint_codes(n, hints)
    zeros = np.zeros(n, dtype=np.float32)
    work = 0
    if all(code):                                                                 # the check pass: every variable has a hint
        bits = [1.0 if c == 1 else 0.0 for c in code]
        reads, ok = check_reads(clauses, bits)
        work += reads
        if ok:
            return 1, np.asarray(bits, dtype=np.float32), work
    val = [0] * n
    trail, mark, dvar = [], {}, {}
    level = 0
    while True:
        if work >= budget:
            return -1, zeros, work
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
        if conflict:
            peak(stats, 'trail', len(trail))
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
                peak(stats, 'undone', len(trail) - mark[level])
                for u in trail[mark[level]:]:
                    val[u] = 0
                del trail[mark[level]:]
                if not second:
                    dvar[level] = (v, True)
                    val[v] = 3 - first
                    trail.append(v)
                    resumed = True
                    break
                level -= 1
            if not resumed:
                return 0, zeros, work
            continue
        if pend:
            continue
        if wmin is None:
            return 1, np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32), work
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
        if code[v]:
            positive = code[v] == 1
        level += 1
        mark[level] = len(trail)
        dvar[level] = (v, False)
        val[v] = 1 if positive else 2
        trail.append(v)


def solve(instances, hints=None, budget=NO_BUDGET):
    "search() over a list: (status int8 [N], models list, work int64 [N])"
    out = [search(n, c, None if hints is None else hints[i], budget) for i, (n, c) in enumerate(instances)]
    return np.array([o[0] for o in out], dtype=np.int8), [o[1] for o in out], np.array([o[2] for o in out], dtype=np.int64)
