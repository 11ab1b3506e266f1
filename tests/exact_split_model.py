"""The split complete search (pdp_exact_solve_split, include/pdp_hip.h) stated in plain Python: one instance answered from 2^depth cubes.

The deciding search of tests/exact_model.py is a deterministic depth-first tree.  A cube is a prefix of that tree: at each of the first
``depth`` decision levels the branch is pinned by one bit of the cube's index (the most significant of the ``depth`` bits belongs to level
1; 0 = the polarity the search tries first, 1 = the other one), and the level counts as already flipped, so backtracking pops through
it.  The 2^depth cubes partition the tree in the order the plain search walks it: the plain search's first model is the model of the
lowest-numbered cube that has one.  Slow: meant for instances of up to about 40 variables."""
import numpy as np

from exact_model import NO_BUDGET, check_reads, hint_codes

MAX_DEPTH = 16
STOPPED = -2          # record of a cube the kernel stopped early because a lower cube had answered 1 (never produced by this model)


def cube(n, clauses, hints, budget, depth, index, spent=0):
    """(status 1 / 0 / -1, model float32 [n], work) of cube ``index`` of the 2^depth cubes: exact_model.search without its check pass and
    with the decisions of levels 1..depth pinned.  ``spent``: reads already on the instance's counter (the rejected check pass's); the
    budget check before every pass is ``spent + work >= budget``, as in the plain search, and ``work`` counts the cube's own reads only."""
    if budget <= 0:
        budget = 1 << 32
    assert 0 <= depth <= MAX_DEPTH and 0 <= index < (1 << depth)
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    code = hint_codes(n, hints)
    zeros = np.zeros(n, dtype=np.float32)
    work = 0
    val = [0] * n
    trail, mark, dvar = [], {}, {}
    level = 0
    while True:
        if spent + work >= budget:
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
        pinned = level <= depth
        if pinned and (index >> (depth - level)) & 1:                             # the cube's bit of this level: the other polarity
            positive = not positive
        mark[level] = len(trail)
        dvar[level] = (v, pinned)                                                 # a pinned level is never flipped
        val[v] = 1 if positive else 2
        trail.append(v)


def search(n, clauses, hints=None, budget=NO_BUDGET, depth=0):
    """(status, model float32 [n], work, first, cubes) of the instance from its 2^depth cubes.  The check pass of exact_model.search runs
    once, under the same condition; if it accepts, that is the answer, first = -1 and no cube runs (cubes = []).  Otherwise first = the
    lowest cube that answers 1 (-1: none); status 1 with that cube's model and work = check reads + the work of cubes 0..first, or
    status 0 if every cube answers 0, else -1, with work = check reads + the work of all cubes.  cubes = [(status, work)] of the cubes
    that count: 0..first, or all."""
    if budget <= 0:
        budget = 1 << 32
    cl = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in cl for l in c])
    code = hint_codes(n, hints)
    work = 0
    if all(code):
        bits = [1.0 if c == 1 else 0.0 for c in code]
        reads, ok = check_reads(cl, bits)
        work += reads
        if ok:
            return 1, np.asarray(bits, dtype=np.float32), work, -1, []
    spent = work
    cubes = []
    for j in range(1 << depth):
        st, model, w = cube(n, cl, hints, budget, depth, j, spent)
        cubes.append((st, w))
        work += w
        if st == 1:
            return 1, model, work, j, cubes
    status = 0 if all(st == 0 for st, _ in cubes) else -1
    return status, np.zeros(n, dtype=np.float32), work, -1, cubes
