"""The optimising complete search (pdp_exact_min_unsat, include/pdp_hip.h) stated in plain Python: status, cost, model, work and
improvements of one instance.

A depth-first branch and bound over the passes of tests/exact_model.py.  The thresholded hint is the first incumbent (``ub`` = the clauses
it leaves unsatisfied); a pass also counts the falsified clauses (``cost``) and the variables asked for in both polarities (``contra``);
``cost + contra >= ub`` prunes, units are forced only where leaving one unsatisfied would reach ``ub``, a state without an open clause is a
better incumbent, and every other state branches -- also on a unit clause.  It counts the same clause-literal reads as csrc/pdp_exact.hip,
so the GPU results can be compared with array_equal.  Slow: meant for instances of up to about 20 variables."""
import numpy as np

from exact_model import NO_BUDGET, peak


def threshold(n, hints):
    "the incumbent a hint stands for: h > 0.5 true, every other value (NaN included) false; no hints: all false"
    if hints is None:
        return [0] * n
    assert len(hints) == n
    return [1 if float(h) > 0.5 else 0 for h in hints]


def unsat_count(clauses, bits):
    "the clauses without a true literal under the 0/1 assignment ``bits``"
    return sum(not any((bits[abs(int(l)) - 1] > 0.5) == (int(l) > 0) for l in c if int(l) != 0) for c in clauses)


def search(n, clauses, hints=None, budget=NO_BUDGET, stats=None):
    """(status 1 / -1, cost, model float32 [n], work, improvements) of the instance (n, clauses: lists of signed 1-based ints) under ``hints``
    ([n] floats or None).  ``stats``: a dict that receives the maxima over the run of ``trail`` (trail length at a prune), ``pass_units``
    (variables one forcing pass assigned), ``pass_cost`` (clauses one pass found falsified) and ``unit_branch`` (1: a decision was taken on
    a clause of width 1); the results do not depend on it."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    bits = threshold(n, hints)
    code = [1 if b else 2 for b in bits]                                          # the first polarity of a decision: the incumbent's
    work, improvements = 0, 0
    # the check pass: every clause up to and including its first true literal; ub = the clauses without one
    ub = 0
    for c in cls:
        k = next((j + 1 for j, (v, want) in enumerate(c) if code[v] == want), None)
        work += len(c) if k is None else k
        ub += k is None
    model = np.asarray(bits, dtype=np.float32)
    if ub == 0:
        return 1, 0, model, work, improvements
    val = [0] * n
    trail, mark, dvar = [], {}, {}
    level = 0
    while True:
        if work >= budget:
            return -1, ub, model, work, improvements
        # one pass: falsified clauses, unit requests, the minimum width of the open clauses (a unit has width 1)
        cost, pend, wmin = 0, {}, None
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
                cost += 1
                continue
            if not distinct:
                pend[first[0]] = pend.get(first[0], 0) | first[1]
            width = nfree if distinct else 1
            wmin = width if wmin is None else min(wmin, width)
        contra = sum(b == 3 for b in pend.values())
        peak(stats, 'pass_cost', cost)
        prune = cost + contra >= ub
        if not prune and cost == ub - 1 and pend:
            # leaving any unit unsatisfied reaches ub: all of them are forced (no variable is asked for twice: that was pruned)
            for v in sorted(pend):
                val[v] = pend[v]
                trail.append(v)
            peak(stats, 'pass_units', len(pend))
            continue
        if not prune and wmin is None:
            # a leaf below ub: the new incumbent
            ub = cost
            improvements += 1
            model = np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32)
            if ub == 0:
                return 1, 0, model, work, improvements
            prune = True
        if prune:
            # chronological backtracking: undo levels until one whose second polarity is untried
            peak(stats, 'trail', len(trail))
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
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
                return 1, ub, model, work, improvements
            continue
        # branching: the unassigned variable with the most occurrences in the open clauses of width wmin, ties to the lower index; the
        # first polarity is the incumbent's
        if wmin == 1:
            peak(stats, 'unit_branch', 1)
        cnt = {}
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
            if sat or nfree == 0 or (nfree if distinct else 1) != wmin:
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
        val[v] = code[v]
        trail.append(v)


def solve(instances, hints=None, budget=NO_BUDGET):
    "search() over a list: (status int8 [N], cost int32 [N], models list, work int64 [N], improvements int32 [N])"
    out = [search(n, c, None if hints is None else hints[i], budget) for i, (n, c) in enumerate(instances)]
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.int32), [o[2] for o in out],
            np.array([o[3] for o in out], dtype=np.int64), np.array([o[4] for o in out], dtype=np.int32))
