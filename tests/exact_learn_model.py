"""The learning complete search (pdp_exact_solve_learn, include/pdp_hip.h) stated in plain Python: status, model, work, learned clauses
and arena reductions of one instance.

It follows csrc/pdp_exact.hip pass by pass like tests/exact_model.py -- the passes, the branching rule, the hint codes, the check pass
and the budget check are that module's -- and replaces chronological backtracking by first-UIP conflict analysis, a learned clause per
conflict and a backjump.  It counts the same clause-literal reads, so the GPU results can be compared with array_equal.  Slow: meant for
small instances (a propagation pass is a Python loop over every clause)."""
import numpy as np

from exact_model import NO_BUDGET, check_reads, hint_codes, peak

NO_ARENA = 1 << 40


def thrash(k):
    """k independent binary clauses on 2 k variables, then the 8 sign patterns over 3 fresh variables: unsatisfiable, and chronological
    backtracking refutes the last three variables again under every combination of the k decisions before them"""
    clauses = [[2 * i + 1, 2 * i + 2] for i in range(k)]
    a = 2 * k + 1
    clauses += [[s0 * a, s1 * (a + 1), s2 * (a + 2)] for s0 in (1, -1) for s1 in (1, -1) for s2 in (1, -1)]
    return 2 * k + 3, clauses


def search(n, clauses, hints=None, budget=NO_BUDGET, arena=0, *, stats=None):
    """(status 1 / 0 / -1, model float32 [n], work, learned, reductions) of the instance (n, clauses: lists of signed 1-based ints) under
    ``hints`` ([n] floats or None).  ``arena``: words for learned clauses (one of len literals takes len + 1), 0 = four per literal of
    the instance.  ``stats``: a dict that receives the maxima over the run of ``trail`` (trail length at a conflict), ``span`` (trail
    slots one analysis walks back), ``gap`` (slots one analysis skips between two variables it resolves on), ``confl_len`` (length of a
    conflict clause or of a reason it is resolved with), ``lc`` (learned-clause length), ``pass_units`` (variables assigned by one pass),
    and per reduction ``live`` (learned clauses before it), ``kept`` (after it), ``kept_idx`` (highest index before it, counted from the
    first learned clause, of a kept one) and ``kept_len`` (longest kept clause); the results do not depend on it."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    m0 = len(cls)
    if arena <= 0:
        arena = 4 * sum(len(c) for c in cls)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    code = hint_codes(n, hints)
    zeros = np.zeros(n, dtype=np.float32)
    work = learned = reductions = used = 0
    if all(code):                                                                 # the check pass: every variable has a hint
        bits = [1.0 if c == 1 else 0.0 for c in code]
        reads, ok = check_reads(clauses, bits)
        work += reads
        if ok:
            return 1, np.asarray(bits, dtype=np.float32), work, 0, 0
    val, lev, rsn = [0] * n, [0] * n, [None] * n
    trail, mark = [], {}
    level = 0
    while True:
        if work >= budget:
            return -1, zeros, work, learned, reductions
        # one unit-propagation pass: the lowest falsified clause, and per literal the lowest clause that asks for it
        confl, req, wmin = None, {}, None
        for ci, c in enumerate(cls):
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
                if confl is None:
                    confl = ci
            elif not distinct:
                req.setdefault(first, ci)
            else:
                wmin = nfree if wmin is None else min(wmin, nfree)
        if confl is None and req:
            asked = sorted({v for v, _ in req})
            both = [v for v in asked if (v, 1) in req and (v, 2) in req]
            before = len(trail)
            for v in asked:
                if both and v == both[0]:
                    val[v], rsn[v], confl = 1, req[(v, 1)], req[(v, 2)]
                elif v in both:
                    continue
                else:
                    val[v] = 1 if (v, 1) in req else 2
                    rsn[v] = req[(v, val[v])]
                lev[v] = level
                trail.append(v)
            peak(stats, 'pass_units', len(trail) - before)
            if confl is None:
                continue
        if confl is not None:
            peak(stats, 'trail', len(trail))
            if level == 0:
                return 0, zeros, work, learned, reductions
            # first-UIP analysis: resolve backwards along the trail until one literal of the current level is left
            seen, out, open_, i, uip = set(), [], 0, len(trail) - 1, None
            c = cls[confl]
            while True:
                work += len(c)
                peak(stats, 'confl_len', len(c))
                for v, p in c:
                    if v in seen:
                        continue
                    seen.add(v)
                    if lev[v] == level:
                        open_ += 1
                    elif lev[v] > 0:
                        out.append((v, p))
                at = i
                while i >= 0 and trail[i] not in seen:
                    i -= 1
                peak(stats, 'gap', at - i)
                assert i >= 0, "a conflict clause without a literal of the current level"
                uip = trail[i]
                i -= 1
                open_ -= 1
                if open_ == 0:
                    break
                c = cls[rsn[uip]]
            lc = [(uip, 3 - val[uip])] + sorted(out)
            peak(stats, 'span', len(trail) - 1 - i)
            peak(stats, 'lc', len(lc))
            bl = max([lev[v] for v, _ in out], default=0)
            for u in trail[mark[bl + 1]:]:
                val[u] = 0
            del trail[mark[bl + 1]:]
            level = bl
            if used + len(lc) + 1 > arena:
                # delete every learned clause that is not the reason of an assigned variable, keep the order, renumber
                reasons = {rsn[v] for v in trail if rsn[v] is not None}
                remap, kept = {}, []
                for ci, c2 in enumerate(cls):
                    if ci < m0 or ci in reasons:
                        remap[ci] = len(kept)
                        kept.append(c2)
                peak(stats, 'live', len(cls) - m0)
                peak(stats, 'kept', len(kept) - m0)
                peak(stats, 'kept_idx', max([ci - m0 for ci in remap if ci >= m0], default=0))
                peak(stats, 'kept_len', max([len(c2) for c2 in kept[m0:]], default=0))
                cls = kept
                for v in trail:
                    if rsn[v] is not None:
                        rsn[v] = remap[rsn[v]]
                used = sum(len(c2) + 1 for c2 in cls[m0:])
                reductions += 1
                if used + len(lc) + 1 > arena:
                    return -1, zeros, work, learned, reductions
            cls.append(lc)
            used += len(lc) + 1
            learned += 1
            continue
        if wmin is None:
            return 1, np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32), work, learned, reductions
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
        val[v], lev[v], rsn[v] = (1 if positive else 2), level, None
        trail.append(v)


def solve(instances, hints=None, budget=NO_BUDGET, arena=0):
    "search() over a list: (status int8 [N], models list, work int64 [N], learned int32 [N], reductions int32 [N])"
    out = [search(n, c, None if hints is None else hints[i], budget, arena) for i, (n, c) in enumerate(instances)]
    return (np.array([o[0] for o in out], dtype=np.int8), [o[1] for o in out], np.array([o[2] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int32), np.array([o[4] for o in out], dtype=np.int32))
