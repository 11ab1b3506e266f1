"""The split nearest-model search (pdp_exact_nearest_split, include/pdp_hip.h) stated in plain Python: one instance's branch and bound
spread over 2^depth cubes that share one word, the cost of the best model found so far.

A cube is tests/exact_nearest_model.py's search with the decisions of levels 1..depth pinned by the bits of the cube's index, exactly as
in tests/exact_split_model.py (the most significant of the ``depth`` bits belongs to level 1; 0 = the hint's polarity, which costs
nothing; 1 = the other one, which adds the variable's penalty to ``dist`` at once; a pinned level counts as already flipped, so
backtracking pops through it and ends the cube).  A pinned decision against the hint that brings ``dist`` to ``live`` ends the cube
before any pass: every open level is pinned, so the flip-time prune of the plain search has nothing left to try.

One bound.  ``live`` is the cube's view of the shared word: its own accepted cost at once, the other cubes' at the next re-read.  A
conflict, a variable asked for twice or ``dist >= live`` prunes, at every level.  Every clause is hard, so the units are always forced
and the branching variable is a function of the assignment alone: the decisions of the pinned levels do not depend on what the other
cubes have found, all cubes agree on one prefix tree whatever the timing, and they partition it.  (tests/exact_min_unsat_split_model.py
needs a second bound, ub0, because its forcing rule reads the bound.)  A prune inside the prefix ends the cube, and a leaf met with fewer
than ``depth`` levels open is reached by every cube that shares those levels' bits: it belongs to the one whose remaining bits are all 0,
the others end there with nothing credited.

The check (once per instance, before the cubes): a penalty outside [0, 2^20] gives status -3 and nothing is searched.  Otherwise the
check pass over the thresholded hint; a hint that is a model sets the shared word to 0.  A start model, when given, is thresholded and
checked by one more such pass (its reads are added to ``chk``); where it satisfies every clause its penalty distance from the hint,
``start_cost``, seeds the shared word and it becomes the model to beat; where it does not it is ignored (``start_cost`` -1).

The shared word is re-read at every budget check, one pass ahead of its use, and once before the cube starts.  ``cube_passes`` is a
generator that yields at every budget check, so that ``interleaved`` can run the cubes of one instance under any schedule; ``sequential``
runs them in ascending order, each to its end, which is what one wave does with PDP_EXACT_GRID=1.  It counts the same clause-literal
reads as csrc/pdp_exact.hip.  Slow."""
import numpy as np

from exact_min_unsat_model import threshold
from exact_model import NO_BUDGET
from exact_nearest_model import MAX_PENALTY, distance, penalty_list

MAX_DEPTH = 16
NO_COST = -1          # cube_cost of a cube that accepted no improvement
INF = (1 << 63) - 1   # the shared word before the first model


def _pass_over(cls, code):
    "(reads, every clause has a true literal): every clause up to and including its first literal that is true under ``code``"
    reads, ok = 0, True
    for c in cls:
        k = next((j + 1 for j, (v, want) in enumerate(c) if code[v] == want), None)
        reads += len(c) if k is None else k
        ok = ok and k is not None
    return reads, ok


def check(n, clauses, hints, penalties, start=None):
    """(n, cls, code, pen, chk, ub, model, start_cost) of the check kernel: ``chk`` the reads (-1: a penalty is out of range, nothing is
    searched), ``ub`` the shared word the cubes start from, ``model`` what stays when no cube accepts anything"""
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    bits = threshold(n, hints)
    code = [1 if b else 2 for b in bits]
    pen = penalty_list(n, penalties)
    zeros = np.zeros(n, dtype=np.float32)
    if any(q < 0 or q > MAX_PENALTY for q in pen):
        return n, cls, code, pen, -1, 0, zeros, -1
    chk, ok = _pass_over(cls, code)
    ub, model = (0, np.asarray(bits, dtype=np.float32)) if ok else (INF, zeros)
    start_cost = -1
    if start is not None:
        sbits = threshold(n, start)
        reads, ok = _pass_over(cls, [1 if b else 2 for b in sbits])
        chk += reads
        if ok:
            start_cost = distance(bits, pen, sbits)
            if start_cost < ub:
                ub, model = start_cost, np.asarray(sbits, dtype=np.float32)
    return n, cls, code, pen, chk, ub, model, start_cost


def cube_passes(n, cls, code, pen, budget, depth, index, chk, shared, out):
    """Generator: cube ``index`` of the 2^depth cubes.  ``shared`` is a one-element list, the instance's shared word.  ``out`` receives
    'status' (1 exhausted / -1 budget spent), 'work' (the cube's own reads), 'cost' (its last accepted cost, NO_COST: none), 'improvements'
    and 'model' (the assignment of that cost, None: none).  Yields before every budget check."""
    assert 0 <= depth <= MAX_DEPTH and 0 <= index < (1 << depth)
    out.update(status=1, work=0, cost=NO_COST, improvements=0, model=None)
    live = shared[0]                                                              # loaded before the instance is copied
    if live == 0:
        return
    seen = live
    work, dist = 0, 0
    val = [0] * n
    trail, mark, dvar, dsnap = [], {}, {}, {}
    level = 0
    while True:
        out['work'] = work
        yield
        live = min(live, seen)
        if live == 0:                                                             # some cube has met the hint's own cost
            return
        if chk + work >= budget:
            out['status'] = -1
            return
        seen = shared[0]                                                          # used at the next check
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
        for v in sorted(pend):
            val[v] = 1 if pend[v] & 1 else 2
            conflict = conflict or pend[v] == 3
            trail.append(v)
            if val[v] != code[v]:
                dist += pen[v]
        prune = conflict or dist >= live
        if not prune and pend:
            continue
        if not prune and wmin is None:
            # a leaf below live; inside the prefix it belongs to the cube whose remaining bits are 0
            if level >= depth or index & ((1 << (depth - level)) - 1) == 0:
                old = shared[0]                                                   # the atomic minimum
                shared[0] = min(old, dist)
                if old > dist:
                    out['cost'] = dist
                    out['improvements'] += 1
                    out['model'] = np.asarray([1.0 if (x or c) == 1 else 0.0 for x, c in zip(val, code)], dtype=np.float32)
                    live = dist
                else:
                    live = old
            prune = True
        if prune:
            # chronological backtracking; a flip that reaches live by its own penalty is pruned at once and the level is undone
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
                for u in trail[mark[level]:]:
                    val[u] = 0
                del trail[mark[level]:]
                dist = dsnap[level]
                if not second and dist + pen[v] < live:
                    dvar[level] = (v, True)
                    val[v] = 3 - first
                    trail.append(v)
                    dist += pen[v]
                    resumed = True
                    break
                level -= 1
            if not resumed:
                out['work'] = work
                return
            continue
        # branching: exact_nearest_model's rule; the first polarity is the hint's, a pinned level takes its bit of the index
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
        pinned = level <= depth
        mark[level] = len(trail)
        dvar[level] = (v, pinned)                                                 # a pinned level is never flipped
        dsnap[level] = dist
        val[v] = code[v]
        trail.append(v)
        if pinned and (index >> (depth - level)) & 1:
            val[v] = 3 - code[v]
            dist += pen[v]
            if dist >= live:                                                      # every open level is pinned: the cube ends
                out['work'] = work
                return


def finish(n, chk, model0, start_cost, shared, outs):
    """(status, cost, model float32 [n], work, improvements, first, start_cost, cubes) from the cubes' records, as the finish kernel: cost =
    the shared word (-1: still infinite), first = the lowest cube whose cost is that (-1: none, what the check wrote stays), cubes =
    [(status, work, cost, improvements)]"""
    cubes = [(o['status'], o['work'], o['cost'], o['improvements']) for o in outs]
    if chk < 0:
        return -3, 0, model0, 0, 0, -1, start_cost, cubes
    cost = -1 if shared[0] == INF else shared[0]
    first = next((j for j, o in enumerate(outs) if o['cost'] == cost and cost >= 0), -1)
    model = model0 if first < 0 else outs[first]['model']
    status = -1 if any(o['status'] != 1 for o in outs) else (1 if cost >= 0 else 0)
    work = chk + sum(o['work'] for o in outs)
    return status, cost, model, work, sum(o['improvements'] for o in outs), first, start_cost, cubes


def _run(n, clauses, hints, penalties, start, budget, depth, order):
    if budget <= 0:
        budget = 1 << 32
    n, cls, code, pen, chk, ub, model0, start_cost = check(n, clauses, hints, penalties, start)
    shared = [ub]
    outs = [{} for _ in range(1 << depth)]
    gens = [cube_passes(n, cls, code, pen, budget, depth, j, chk, shared, outs[j]) for j in range(1 << depth)]
    order(gens)
    return finish(n, chk, model0, start_cost, shared, outs)


def sequential(n, clauses, hints=None, penalties=None, start=None, budget=NO_BUDGET, depth=0):
    "the cubes in ascending order, each to its end: one wave (PDP_EXACT_GRID=1)"
    def order(gens):
        for g in gens:
            for _ in g:
                pass
    return _run(n, clauses, hints, penalties, start, budget, depth, order)


def interleaved(n, clauses, hints=None, penalties=None, start=None, budget=NO_BUDGET, depth=0, seed=0, width=8):
    """a random schedule: up to ``width`` cubes are in flight, taken in ascending order as the counter hands them out; at every step one of
    them, chosen at random, runs one pass"""
    rng = np.random.RandomState(seed)

    def order(gens):
        waiting, flying = list(gens), []
        while waiting or flying:
            while waiting and len(flying) < width:
                flying.append(waiting.pop(0))
            k = rng.randint(len(flying))
            try:
                next(flying[k])
            except StopIteration:
                flying.pop(k)
    return _run(n, clauses, hints, penalties, start, budget, depth, order)


def solve(instances, hints=None, penalties=None, starts=None, budget=NO_BUDGET, depths=0):
    "sequential() over a list (depths: an int or one per instance; starts: None or a list with None where there is none): a list of its tuples"
    if isinstance(depths, int):
        depths = [depths] * len(instances)
    return [sequential(n, c, None if hints is None else hints[i], None if penalties is None else penalties[i],
                       None if starts is None else starts[i], budget, int(d)) for i, ((n, c), d) in enumerate(zip(instances, depths))]
