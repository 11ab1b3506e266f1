"""The split optimising search (pdp_exact_min_unsat_split, include/pdp_hip.h) stated in plain Python: one instance's branch and bound
spread over 2^depth cubes that share one word, the best cost found so far.

A cube is tests/exact_min_unsat_model.py's search with the decisions of levels 1..depth pinned by the bits of the cube's index, exactly as
in tests/exact_split_model.py (the most significant of the ``depth`` bits belongs to level 1; 0 = the polarity the search tries first, the
hint's; 1 = the other one; a pinned level counts as already flipped, so backtracking pops through it and ends the cube).

Two bounds.  ``live`` is the cube's view of the shared word: its own accepted cost at once, the other cubes' at the next re-read.  Every
pass prunes on ``cost + contra >= live``.  Forcing all units (``cost == rule - 1``) uses ``rule``: ``ub0``, the thresholded hint's cost,
while ``level < depth``, and ``live`` from then on.  The decisions of the pinned levels are therefore taken in states that depend on the
instance and its hint alone, whatever the other cubes have found by then: all cubes agree on the prefix tree, and they partition it.
(Forcing under ub0 is sound because live <= ub0; not forcing merely leaves a unit to a pinned decision.)  A prune inside the prefix ends
the cube -- every open level is pinned -- and a leaf met with fewer than ``depth`` levels open is reached by every cube that shares those
levels' bits: it belongs to the one whose remaining bits are all 0, the others end there with nothing credited.

The shared word is re-read at every budget check, one pass ahead of its use (the value loaded before pass k is used at the check before
pass k + 1), and once before the cube starts.  ``cube_passes`` is a generator that yields at every point where the other cubes' progress
can matter, so that ``interleaved`` can run the cubes of one instance under any schedule; ``sequential`` runs them in ascending order, each
to its end, which is what one wave does with PDP_EXACT_GRID=1.  It counts the same clause-literal reads as csrc/pdp_exact.hip.  Slow."""
import numpy as np

from exact_min_unsat_model import threshold
from exact_model import NO_BUDGET

MAX_DEPTH = 16
NO_COST = -1          # cube_cost of a cube that accepted no improvement


def check(n, clauses, hints):
    "(n, cls, code, bits, chk, ub0): the check pass -- every clause up to and including its first true literal under the thresholded hint"
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    bits = threshold(n, hints)
    code = [1 if b else 2 for b in bits]
    chk, ub0 = 0, 0
    for c in cls:
        k = next((j + 1 for j, (v, want) in enumerate(c) if code[v] == want), None)
        chk += len(c) if k is None else k
        ub0 += k is None
    return n, cls, code, bits, chk, ub0


def cube_passes(n, cls, code, budget, depth, index, chk, ub0, shared, out):
    """Generator: cube ``index`` of the 2^depth cubes.  ``shared`` is a one-element list, the instance's shared word.  ``out`` receives
    'status' (1 exhausted / -1 budget spent), 'work' (the cube's own reads), 'cost' (its last accepted cost, NO_COST: none), 'improvements'
    and 'model' (the assignment of that cost, None: none).  Yields before every budget check."""
    assert 0 <= depth <= MAX_DEPTH and 0 <= index < (1 << depth)
    out.update(status=1, work=0, cost=NO_COST, improvements=0, model=None)
    live = shared[0]                                                              # loaded before the instance is copied
    if live == 0:
        return
    seen = live
    work = 0
    val = [0] * n
    trail, mark, dvar = [], {}, {}
    level = 0
    while True:
        out['work'] = work
        yield
        live = min(live, seen)
        if live == 0:                                                             # some cube has satisfied every clause
            return
        if chk + work >= budget:
            out['status'] = -1
            return
        seen = shared[0]                                                          # used at the next check
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
        rule = ub0 if level < depth else live
        prune = cost + contra >= live
        if not prune and cost == rule - 1 and pend:
            for v in sorted(pend):
                val[v] = pend[v]
                trail.append(v)
            continue
        if not prune and wmin is None:
            # a leaf below live; inside the prefix it belongs to the cube whose remaining bits are 0
            if level >= depth or index & ((1 << (depth - level)) - 1) == 0:
                old = shared[0]                                                   # the atomic minimum
                shared[0] = min(old, cost)
                if old > cost:
                    out['cost'] = cost
                    out['improvements'] += 1
                    out['model'] = np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32)
                    live = cost
                else:
                    live = old
            prune = True
        if prune:
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
                out['work'] = work
                return
            continue
        # branching: exact_min_unsat_model's rule; the first polarity is the hint's, a pinned level takes its bit of the index
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
        pinned = level <= depth
        pol = code[v]
        if pinned and (index >> (depth - level)) & 1:
            pol = 3 - pol
        mark[level] = len(trail)
        dvar[level] = (v, pinned)                                                 # a pinned level is never flipped
        val[v] = pol
        trail.append(v)


def finish(n, bits, chk, ub0, shared, outs):
    """(status, cost, model float32 [n], work, improvements, first, cubes) from the cubes' records, as the finish kernel: cost = the shared
    word, first = the lowest cube whose cost is that (-1: none, the thresholded hint stays), cubes = [(status, work, cost, improvements)]"""
    cost = shared[0]
    first = next((j for j, o in enumerate(outs) if o['cost'] == cost), -1)
    model = np.asarray(bits, dtype=np.float32) if first < 0 else outs[first]['model']
    status = 1 if all(o['status'] == 1 for o in outs) else -1
    work = chk + sum(o['work'] for o in outs)
    return (status, cost, model, work, sum(o['improvements'] for o in outs), first,
            [(o['status'], o['work'], o['cost'], o['improvements']) for o in outs])


def _run(n, clauses, hints, budget, depth, order):
    if budget <= 0:
        budget = 1 << 32
    n, cls, code, bits, chk, ub0 = check(n, clauses, hints)
    shared = [ub0]
    outs = [{} for _ in range(1 << depth)]
    gens = [cube_passes(n, cls, code, budget, depth, j, chk, ub0, shared, outs[j]) for j in range(1 << depth)]
    order(gens)
    return finish(n, bits, chk, ub0, shared, outs)


def sequential(n, clauses, hints=None, budget=NO_BUDGET, depth=0):
    "the cubes in ascending order, each to its end: one wave (PDP_EXACT_GRID=1)"
    def order(gens):
        for g in gens:
            for _ in g:
                pass
    return _run(n, clauses, hints, budget, depth, order)


def interleaved(n, clauses, hints=None, budget=NO_BUDGET, depth=0, seed=0, width=8):
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
    return _run(n, clauses, hints, budget, depth, order)


def solve(instances, hints=None, budget=NO_BUDGET, depths=0):
    "sequential() over a list (depths: an int or one per instance): a list of its tuples"
    if isinstance(depths, int):
        depths = [depths] * len(instances)
    return [sequential(n, c, None if hints is None else hints[i], budget, int(d)) for i, ((n, c), d) in enumerate(zip(instances, depths))]
