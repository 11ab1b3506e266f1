"""The k-th model of the counting complete search (pdp_exact_models_at, include/pdp_hip.h) stated in plain Python: status, count_seen,
found, models, work and leaves of one instance and one non-decreasing list of ranks.

tests/exact_count_model.py's search with a cursor over ``ranks`` and without T, F, snap and the crediting.  The counting search meets its
leaves (satisfying cubes) in a fixed depth-first order and a leaf with f unassigned variables stands for 2^f models, so "count before
the leaf + offset inside it" numbers every model once.  At a leaf, before = count, count = count + ldexp(1.0, n - trail length), and
every rank r with r < count that is still unanswered is emitted: o = r - before in integers (both below 2^53: exact), an assigned
variable takes its value, the j-th unassigned variable in ascending index (j from 0) takes bit j of o, bits from 53 up are 0.  When the
last rank is answered the search ends there with status 1, before any backtracking.  Emitting costs no work: work counts clause-literal
reads only.  Out of levels: status 1, the unanswered ranks get found = 0 ("there is no such model") and a row of zeros; out of budget:
status -1, found = -1 and a row of zeros.  n > 1023: status -2, nothing searched, every found -1; no ranks: status 1, nothing searched.

Consequences (tests/test_exact_rank_host.py asserts them):
 (a) ranks 0 .. count-1 enumerate the models of a complete count, each once;
 (b) a call with a rank >= the instance's count has the work, leaves and count_seen of the counting search; every other call has work
     and leaves at most those;
 (c) every answer is a function of the instance and the rank alone: the model of a rank does not depend on the other ranks asked for,
     and under a smaller budget a rank is either answered with the same model or gets found = -1.
Slow: meant for small instances."""
import math

import numpy as np

from exact_model import NO_BUDGET

MAX_N = 1023            # as exact_count_model: a larger instance gets status -2
MAX_RANK = 1 << 53      # ranks are below this: every rank and every count a rank is compared with are exact doubles


def search(n, clauses, ranks, budget=NO_BUDGET):
    """(status 1 / -1 / -2, count_seen float, found int8 [K], models uint8 [K, n], work, leaves) of the instance (n, clauses: lists of
    signed 1-based ints) for ``ranks``: K non-decreasing ints in [0, 2^53)."""
    if budget <= 0:
        budget = 1 << 32
    ranks = [int(r) for r in ranks]
    assert all(0 <= r < MAX_RANK for r in ranks) and all(a <= b for a, b in zip(ranks, ranks[1:])), "ranks: non-decreasing, in [0, 2^53)"
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    K = len(ranks)
    found = np.zeros(K, dtype=np.int8)
    models = np.zeros((K, n), dtype=np.uint8)
    if n > MAX_N:
        found[:] = -1
        return -2, 0.0, found, models, 0, 0
    if K == 0:
        return 1, 0.0, found, models, 0, 0
    work, leaves, count, cur = 0, 0, 0.0, 0
    val = [0] * n
    trail, mark, dvar = [], {0: 0}, {}
    level = 0
    status = 1
    while True:
        if work >= budget:
            status = -1
            break
        # one unit-propagation pass (exact_count_model's)
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
            # a leaf: the ranks in [before, count) are its models
            before = count
            count = count + math.ldexp(1.0, n - len(trail))
            leaves += 1
            while cur < K and ranks[cur] < count:
                o = ranks[cur] - int(before)
                j = 0
                for v in range(n):
                    if val[v] == 0:
                        models[cur, v] = (o >> j) & 1 if j < 53 else 0
                        j += 1
                    else:
                        models[cur, v] = 1 if val[v] == 1 else 0
                found[cur] = 1
                cur += 1
            if cur == K:
                break
            conflict = True
        if conflict:
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
                break
            continue
        # branching (exact_count_model's)
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
        val[v] = 1 if positive else 2
        trail.append(v)
    if status == -1:
        found[cur:] = -1
    return status, count, found, models, work, leaves


def solve(instances, ranks, budget=NO_BUDGET):
    """search() over lists: (status int8 [N], count_seen float64 [N], found list, models list, work int64 [N], leaves int64 [N])"""
    out = [search(n, c, r, budget) for (n, c), r in zip(instances, ranks)]
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.float64), [o[2] for o in out],
            [o[3] for o in out], np.array([o[4] for o in out], dtype=np.int64), np.array([o[5] for o in out], dtype=np.int64))
