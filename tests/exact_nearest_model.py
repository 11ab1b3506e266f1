"""The nearest-model search (pdp_exact_nearest, include/pdp_hip.h) stated in plain Python: status, cost, model, work and improvements of
one instance.

A depth-first branch and bound over the passes of tests/exact_model.py with the cost on the variables and every clause hard.  The
thresholded hint is the point the distance is measured from: ``cost(x)`` is the sum of ``pen[v]`` over the variables with
``x[v] != bits[v]`` (all penalties 1: the Hamming distance).  ``dist`` is the cost of the assigned variables; ``dist >= ub`` prunes, a
state without an open clause is a model of cost ``dist`` (the unassigned variables take their hint values, which cost nothing), the
first polarity of a decision is the hint's, and a flip whose penalty alone reaches ``ub`` is pruned before any pass.  It counts the same
clause-literal reads as csrc/pdp_exact.hip, so the GPU results can be compared with array_equal.  Slow: meant for instances of up to
about 20 variables."""
import numpy as np

from exact_min_unsat_model import threshold
from exact_model import NO_BUDGET, peak

MAX_PENALTY = 1 << 20


def penalty_list(n, penalties):
    "the penalties as n Python ints (None: all 1)"
    if penalties is None:
        return [1] * n
    assert len(penalties) == n
    return [int(q) for q in penalties]


def distance(bits, pen, model):
    "the penalty sum over the variables where the 0/1 ``model`` differs from ``bits``"
    return sum(q for b, q, x in zip(bits, pen, model) if (float(x) > 0.5) != bool(b))


def search(n, clauses, hints=None, penalties=None, budget=NO_BUDGET, stats=None):
    """(status 1 / 0 / -1 / -3, cost, model float32 [n], work, improvements) of the instance (n, clauses: lists of signed 1-based ints)
    under ``hints`` ([n] floats or None) and ``penalties`` ([n] ints in [0, 2^20] or None).  Status -3: a penalty is out of range, nothing
    is searched and every other output is 0.  ``stats``: a dict that receives the maxima over the run of ``trail`` (trail length at a
    prune), ``pass_units`` (variables one pass assigned), ``pass_against`` (of those, the ones assigned against the hint), ``undone``
    (trail entries cleared by one backtrack step), ``fill`` (unassigned variables with a true hint at a leaf) and ``flip_pruned`` (1: a flip
    was pruned before any pass); the results do not depend on it."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    bits = threshold(n, hints)
    code = [1 if b else 2 for b in bits]                                          # the hint's value: the first polarity of a decision
    pen = penalty_list(n, penalties)
    zeros = np.zeros(n, dtype=np.float32)
    if any(q < 0 or q > MAX_PENALTY for q in pen):
        return -3, 0, zeros, 0, 0
    work, improvements = 0, 0
    # the check pass: every clause up to and including its first literal that is true under the hint
    ok = True
    for c in cls:
        k = next((j + 1 for j, (v, want) in enumerate(c) if code[v] == want), None)
        work += len(c) if k is None else k
        ok = ok and k is not None
    if ok:
        return 1, 0, np.asarray(bits, dtype=np.float32), work, improvements
    ub, model = None, zeros                                                       # None: infinity, no model met yet
    dist = 0
    val = [0] * n
    trail, mark, dvar, dsnap = [], {}, {}, {}
    level = 0
    while True:
        if work >= budget:
            return -1, (-1 if ub is None else ub), model, work, improvements
        # one pass of tests/exact_model.py: conflict flag, unit requests, wmin over the open non-unit clauses
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
        against = 0
        for v in sorted(pend):
            val[v] = 1 if pend[v] & 1 else 2
            conflict = conflict or pend[v] == 3
            trail.append(v)
            if val[v] != code[v]:
                dist += pen[v]
                against += 1
        peak(stats, 'pass_units', len(pend))
        peak(stats, 'pass_against', against)
        prune = conflict or (ub is not None and dist >= ub)
        if not prune and pend:
            continue
        if not prune and wmin is None:
            # a leaf below ub: the unassigned variables take their hint values and cost nothing
            ub = dist
            improvements += 1
            model = np.asarray([1.0 if (x or c) == 1 else 0.0 for x, c in zip(val, code)], dtype=np.float32)
            peak(stats, 'fill', sum(x == 0 and c == 1 for x, c in zip(val, code)))
            if ub == 0:
                return 1, 0, model, work, improvements
            prune = True
        if prune:
            # chronological backtracking; a flip that reaches ub by its own penalty is pruned at once and the level is undone
            peak(stats, 'trail', len(trail))
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
                peak(stats, 'undone', len(trail) - mark[level])
                for u in trail[mark[level]:]:
                    val[u] = 0
                del trail[mark[level]:]
                dist = dsnap[level]
                if not second:
                    if ub is not None and dist + pen[v] >= ub:
                        peak(stats, 'flip_pruned', 1)
                    else:
                        dvar[level] = (v, True)
                        val[v] = 3 - first
                        trail.append(v)
                        dist += pen[v]
                        resumed = True
                        break
                level -= 1
            if not resumed:
                if ub is None:
                    return 0, -1, zeros, work, improvements
                return 1, ub, model, work, improvements
            continue
        # branching: the unassigned variable with the most occurrences in the open clauses of width wmin, ties to the lower index; the
        # first polarity is the hint's and costs nothing
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
        level += 1
        mark[level] = len(trail)
        dvar[level] = (v, False)
        dsnap[level] = dist
        val[v] = code[v]
        trail.append(v)


def solve(instances, hints=None, penalties=None, budget=NO_BUDGET):
    "search() over a list: (status int8 [N], cost int64 [N], models list, work int64 [N], improvements int32 [N])"
    out = [search(n, c, None if hints is None else hints[i], None if penalties is None else penalties[i], budget)
           for i, (n, c) in enumerate(instances)]
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.int64), [o[2] for o in out],
            np.array([o[3] for o in out], dtype=np.int64), np.array([o[4] for o in out], dtype=np.int32))
