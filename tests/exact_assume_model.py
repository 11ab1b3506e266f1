"""The learning complete search under assumptions (pdp_exact_solve_learn_assume, include/pdp_hip.h) stated in plain Python: status, model,
work, learned clauses, arena reductions and the failed set of one instance.

It is tests/exact_learn_model.py's search -- the passes, the requests, the first-UIP analysis, the backjump, the arena rule, the branching
rule, the hint codes and the budget check are restated here line by line, and with no assumption nothing else runs -- with the three
additions of the specification: the hint code of an assumed variable is the assumption, level 1 belongs to the assumptions and is opened
at every fixed point of level 0, and a conflict at level 1 ends the search with the final analysis, which collects the assumptions the
conflict rests on.  It counts the same clause-literal reads as the kernel, so the GPU results can be compared with array_equal.  Slow:
meant for small instances.  ``backbone`` states what pdp.exact.backbone computes, ``brute`` is the enumeration the tests judge both by."""
import itertools

import numpy as np

from exact_learn_model import NO_ARENA, thrash  # noqa: F401  (re-exported for the tests)
from exact_model import NO_BUDGET, check_reads, hint_codes, peak


def assume_codes(n, assume):
    "0 not assumed, 1 assumed true (a > 0), 2 assumed false (a < 0)"
    if assume is None:
        return [0] * n
    assert len(assume) == n
    return [1 if int(a) > 0 else (2 if int(a) < 0 else 0) for a in assume]


def search(n, clauses, hints=None, assume=None, budget=NO_BUDGET, arena=0, *, stats=None):
    """(status 1 / 0 / -1, model float32 [n], work, learned, reductions, failed) of the instance (n, clauses: lists of signed 1-based ints)
    under ``hints`` ([n] floats or None) and ``assume`` ([n] integers: > 0 assumed true, < 0 assumed false, 0 not assumed; or None).
    ``failed``: the 0-based variables of the failed set, ascending (an int64 array; empty unless status is 0).  ``arena`` as in
    exact_learn_model.search.  ``stats``: a dict that receives that search's maxima and those of ``assumed`` (variables assigned by one
    opening of level 1), ``opens`` (how often level 1 was opened), ``final_span`` (trail slots the final analysis walks: the trail above
    mark[1]), ``final_len`` (the longest clause it resolves with, the conflict clause included), ``failed`` (the size of the failed
    set), ``live_l1`` (per reduction: level-1 variables whose reason is a learned clause); the results do not depend on it."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    m0 = len(cls)
    if arena <= 0:
        arena = 4 * sum(len(c) for c in cls)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    code = hint_codes(n, hints)
    want = assume_codes(n, None if assume is None else list(assume) + [0] * (n - len(assume)))
    assumed = [v for v in range(n) if want[v]]
    for v in assumed:
        code[v] = want[v]                                                         # the effective code
    none = np.zeros(0, dtype=np.int64)
    zeros = np.zeros(n, dtype=np.float32)
    work = learned = reductions = used = opens = 0
    if all(code):                                                                 # the check pass: every variable has a code
        bits = [1.0 if c == 1 else 0.0 for c in code]
        reads, ok = check_reads(clauses, bits)
        work += reads
        if ok:
            return 1, np.asarray(bits, dtype=np.float32), work, 0, 0, none
    val, lev, rsn = [0] * n, [0] * n, [None] * n
    trail, mark = [], {}
    level = 0
    while True:
        if work >= budget:
            return -1, zeros, work, learned, reductions, none
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
                return 0, zeros, work, learned, reductions, none
            if assumed and level == 1:
                # the final analysis: backwards along the trail down to mark[1], resolving every seen variable that has a reason
                seen, failed, i = set(), [], len(trail) - 1
                c = cls[confl]
                peak(stats, 'final_span', len(trail) - mark[1])
                while c is not None:
                    work += len(c)
                    peak(stats, 'final_len', len(c))
                    seen.update(v for v, _ in c if lev[v] == 1)
                    c = None
                    while i >= mark[1] and c is None:
                        u = trail[i]
                        i -= 1
                        if u in seen:
                            if rsn[u] is None:
                                failed.append(u)
                            else:
                                c = cls[rsn[u]]
                peak(stats, 'failed', len(failed))
                return 0, zeros, work, learned, reductions, np.asarray(sorted(failed), dtype=np.int64)
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
                if assumed:
                    peak(stats, 'live_l1', sum(1 for v in trail if lev[v] == 1 and rsn[v] is not None and rsn[v] >= m0))
                cls = kept
                for v in trail:
                    if rsn[v] is not None:
                        rsn[v] = remap[rsn[v]]
                used = sum(len(c2) + 1 for c2 in cls[m0:])
                reductions += 1
                if used + len(lc) + 1 > arena:
                    return -1, zeros, work, learned, reductions, none
            cls.append(lc)
            used += len(lc) + 1
            learned += 1
            continue
        if assumed and level == 0:
            # the fixed point of level 0: level 1 takes the assumptions.  No clause literal is read.
            level = 1
            mark[1] = len(trail)
            opens += 1
            peak(stats, 'opens', opens)
            against = [v for v in assumed if val[v] and val[v] != want[v]]
            if against:
                peak(stats, 'failed', 1)
                return 0, zeros, work, learned, reductions, np.asarray(against[:1], dtype=np.int64)
            for v in assumed:
                if val[v] == 0:
                    val[v], lev[v], rsn[v] = want[v], 1, None
                    trail.append(v)
            peak(stats, 'assumed', len(trail) - mark[1])
            continue
        if wmin is None:
            return 1, np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32), work, learned, reductions, none
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


def solve(instances, hints=None, assume=None, budget=NO_BUDGET, arena=0, stats=None):
    """search() over a list: (status int8 [N], models list, work int64 [N], learned int32 [N], reductions int32 [N], failed list of int64
    arrays).  ``stats``: a list that receives one dict per instance."""
    out = []
    for i, (n, c) in enumerate(instances):
        st = None if stats is None else {}
        out.append(search(n, c, None if hints is None else hints[i], None if assume is None else assume[i], budget, arena, stats=st))
        if stats is not None:
            stats.append(st)
    return (np.array([o[0] for o in out], dtype=np.int8), [o[1] for o in out], np.array([o[2] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int32), np.array([o[4] for o in out], dtype=np.int32), [o[5] for o in out])


def units(n, clauses, assume, only=None):
    "the instance with the assumptions (``only``: just these 0-based variables) appended as unit clauses"
    pick = range(n) if only is None else [int(v) for v in only]
    return n, [list(c) for c in clauses] + [[(v + 1) if int(assume[v]) > 0 else -(v + 1)] for v in pick if int(assume[v]) != 0]


def brute(n, clauses):
    "every model of the instance by enumeration: a bool array [models, n] (n <= 16 or so)"
    n = max([n] + [abs(int(l)) for c in clauses for l in c])
    grid = np.array(list(itertools.product((False, True), repeat=n)), dtype=bool).reshape(-1, n)
    ok = np.ones(len(grid), dtype=bool)
    for c in clauses:
        sat = np.zeros(len(grid), dtype=bool)
        for l in c:
            if int(l) != 0:
                sat |= grid[:, abs(int(l)) - 1] == (int(l) > 0)
        ok &= sat
    return grid[ok]


def backbone(n, clauses, budget=NO_BUDGET, arena=0):
    """(status, backbone) as pdp.exact.backbone defines them: with M the model of the base search, v is in the backbone iff the instance is
    unsatisfiable under the single assumption v = not M[v].  int8 [n]: +1 true in every model, -1 false in every model, 0 free, 2 not
    decided within the budget; None unless the base search answers 1."""
    st, model = search(n, clauses, None, None, budget, arena)[:2]
    if st != 1:
        return st, None
    out = np.zeros(len(model), dtype=np.int8)
    for v in range(len(model)):
        a = np.zeros(len(model), dtype=np.int8)
        a[v] = -1 if model[v] > 0.5 else 1
        q = search(n, clauses, None, a, budget, arena)[0]
        out[v] = (1 if model[v] > 0.5 else -1) if q == 0 else (0 if q == 1 else 2)
    return st, out
