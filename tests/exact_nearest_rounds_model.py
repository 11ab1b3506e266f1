"""The resumable nearest-model search (pdp_exact_nearest_round, then pdp_exact_count_expand; include/pdp_hip.h) stated in plain Python.

The frontier is tests/exact_count_rounds_model.py's, unchanged: a cube is a path of (bit, closed) pairs, one per decision level, and
``children``, ``pack``, ``unpack``, ``words`` and ``frontier`` are that module's.  ``cube`` is the branch and bound of
tests/exact_nearest_model.py without its check pass, with the decisions of the path's levels taken from the path (bit 0: the hint's
polarity, which costs nothing; bit 1: the other, which costs the variable's penalty at once), the round budget of the counting rounds
-- tested only where a node begins, the replay of the path free against it -- and, at a budget stop, the checkpoint.  The bound ``ub``
is the instance's cost when the round began and appears in the prune only: the units are always forced and the branching variable
does not read it, so the tree a path is replayed in does not depend on it, and a checkpoint written under one bound is replayed under
a lower one either identically or pruned earlier.  ``round`` runs a whole frontier and exchanges the bound: every cube of an instance
starts from ``cost[b]``, the instance takes the minimum of its cubes' costs and the model of the lowest cube that holds it, and the
next round hands that to every cube.  No cube reads a word of another inside a round, so every record is a function of the inputs.

Where the plain call's check pass accepts the hint, this search follows the hint to a leaf of cost 0: status 1, cost 0, model = the
thresholded hint, and one improvement where the plain call reports none.  Slow: meant for small instances."""
import numpy as np

from exact_count_rounds_model import MAX_CUBES, MAX_N, check_path, children, frontier, inst_n, pack, unpack, words  # noqa: F401
from exact_min_unsat_model import threshold
from exact_nearest_model import MAX_PENALTY, distance, penalty_list  # noqa: F401

ROUND_BUDGET = 1 << 18         # PDP_EXACT_NEAREST_ROUND_BUDGET: the reads per cube and round when budget <= 0
DROPPED = -2                   # record of a stopped cube whose instance has reached cost 0
BAD_PENALTY = -3


def cube(n, clauses, hints, penalties, path, budget, ub, stats=None):
    """(status 1 / -1, cube_cost, model float32 [n], work, replay, improvements, checkpoint) of one cube under the bound ``ub`` (None:
    infinite).  Status 1: ended, nothing below the bound it ran under is left in it; -1: stopped, with a checkpoint.  ``cube_cost`` is
    the cost of the last leaf it accepted, -1 if none (model zeros then).  ``stats``: a dict whose 'in_replay' is set to 1 when the
    cube ended before the first node past its path began; the results do not depend on it."""
    if budget <= 0:
        budget = ROUND_BUDGET
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    assert n <= MAX_N
    check_path(n, path)
    bits = threshold(n, hints)
    code = [1 if b else 2 for b in bits]
    pen = penalty_list(n, penalties)
    assert all(0 <= q <= MAX_PENALTY for q in pen)
    model = np.zeros(n, dtype=np.float32)
    work, improvements, cube_cost, dist = 0, 0, -1, 0
    val = [0] * n
    trail, mark, dvar, other, dsnap = [], {}, {}, {}, {}
    level, plen, base, fresh = 0, len(path), None, True
    at_once = False                                                               # a bit-1 decision has reached ub: no pass is made

    def done(status, checkpoint=None):
        if stats is not None and status == 1 and base is None:
            stats['in_replay'] = 1
        return status, cube_cost, model, work, (work if base is None else base), improvements, checkpoint

    while True:
        prune = at_once
        at_once = False
        pend, wmin = {}, None
        if not prune:
            if fresh:
                # a node begins: the first one with level >= plen starts the budget's clock, every one tests it
                if base is None and level >= plen:
                    base = work
                if base is not None and work - base >= budget:
                    return done(-1, [(other[L], int(dvar[L][1])) for L in range(1, level + 1)])
                fresh = False
            # one unit-propagation pass
            conflict = False
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
            prune = conflict or (ub is not None and dist >= ub)
            if not prune and pend:
                continue
            if not prune and wmin is None:
                # a leaf below ub, wherever it is met (inside the path too): the unassigned variables take their hint values
                ub = cube_cost = dist
                improvements += 1
                model = np.asarray([1.0 if (x or c) == 1 else 0.0 for x, c in zip(val, code)], dtype=np.float32)
                if ub == 0:
                    return done(1)
                prune = True
        if prune:
            # chronological backtracking; a flip that reaches ub by its own penalty is skipped and the level undone
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
                for u in trail[mark[level]:]:
                    val[u] = 0
                del trail[mark[level]:]
                dist = dsnap[level]
                if not second and not (ub is not None and dist + pen[v] >= ub):
                    dvar[level] = (v, True)
                    other[level] = 1
                    val[v] = 3 - first
                    trail.append(v)
                    dist += pen[v]
                    resumed = True
                    break
                level -= 1
            if not resumed:
                return done(1)
            plen = min(plen, level)                                               # the path beyond a flipped level no longer applies
            fresh = True
            continue
        # branching: the unassigned variable with the most occurrences in the open clauses of width wmin, ties to the lower index
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
        bit, closed = path[level - 1] if level <= plen else (0, 0)
        mark[level] = len(trail)
        dvar[level] = (v, bool(closed))
        other[level] = int(bit)
        dsnap[level] = dist
        val[v] = 3 - code[v] if bit else code[v]
        trail.append(v)
        if bit:
            # against the hint: the penalty counts at once, and a state that reaches ub is pruned before any pass
            dist += pen[v]
            at_once = ub is not None and dist >= ub
        fresh = True


class State:
    """The answers and the open frontier of a batch: ``paths[b]`` the open cubes of instance b in cube order, ``status`` [B] (-1 open, 1,
    0, -2 not searched, -3 a penalty out of range), ``cost`` [B] (-1: no model yet), ``model`` a list of float32 arrays, ``work``,
    ``improvements`` and ``rounds`` [B].  ``start``: per instance a 0/1 array or None; it seeds cost and model only where it is a model."""

    def __init__(self, instances, hints=None, penalties=None, start=None):
        B = len(instances)
        self.n = [inst_n(i) for i in instances]
        self.hints, self.penalties = hints, penalties
        self.status, self.paths = [], []
        for b, n in enumerate(self.n):
            pen = penalty_list(n, self.pen(b))
            bad = any(q < 0 or q > MAX_PENALTY for q in pen)
            self.status.append(BAD_PENALTY if bad else (-1 if n <= MAX_N else -2))
            self.paths.append([[]] if self.status[b] == -1 else [])
        self.cost = [-1] * B
        self.model = [np.zeros(n, dtype=np.float32) for n in self.n]
        self.work = [0] * B
        self.improvements = [0] * B
        self.rounds = [0] * B
        if start is not None:
            for b, (n, clauses) in enumerate(instances):
                if start[b] is None or self.status[b] != -1:
                    continue
                x = threshold(self.n[b], start[b])
                if all(any((l > 0) == bool(x[abs(l) - 1]) for l in c if l != 0) for c in clauses):
                    self.cost[b] = distance(threshold(self.n[b], self.hint(b)), penalty_list(self.n[b], self.pen(b)), x)
                    self.model[b] = np.asarray(x, dtype=np.float32)

    def cubes(self):
        return sum(len(p) for p in self.paths)

    def hint(self, b):
        return None if self.hints is None else self.hints[b]

    def pen(self, b):
        return None if self.penalties is None else self.penalties[b]


def round(instances, state, budget=0, give=0, whole=(), stats=None):
    """One round: every open cube runs for ``budget`` reads past its replay under the bound cost[b] of its instance; then the outcome of
    every instance that has cubes, and the frontier becomes the expansion of the cubes that are still stopped.  ``whole``: the instances
    that are never expanded (the HBM route's).  Returns (records [(instance, status, cube_cost, work, replay, improvements, checkpoint)]
    in cube order, first [B]: the lowest cube of the instance, counted from its own first one, that holds the instance's new cost; -1:
    the cost did not fall, or no cube).  ``stats``: a dict that counts 'in_replay', the cubes that ended inside the replay of their
    path."""
    records, first = [], [-1] * len(instances)
    nxt = 0
    for b, (n, clauses) in enumerate(instances):
        if not state.paths[b]:
            continue
        state.rounds[b] += 1
        ub = None if state.cost[b] < 0 else state.cost[b]
        mine, models = [], []
        for path in state.paths[b]:
            cs = {}
            st, cc, model, w, replay, imp, cp = cube(n, clauses, state.hint(b), state.pen(b), path, budget, ub, cs)
            if stats is not None and cs.get('in_replay') and path:
                stats['in_replay'] = stats.get('in_replay', 0) + 1
            state.work[b] += w
            state.improvements[b] += imp
            mine.append([b, st, cc, w, replay, imp, cp or []])
            models.append(model)
        found = [r[2] for r in mine if r[2] >= 0]
        if found and (state.cost[b] < 0 or min(found) < state.cost[b]):
            state.cost[b] = min(found)
            first[b] = next(j for j, r in enumerate(mine) if r[2] == state.cost[b])
            state.model[b] = models[first[b]]
        new = []
        if state.cost[b] == 0:
            state.status[b] = 1
            for r in mine:
                if r[1] == -1:
                    r[1] = DROPPED                                                # its checkpoint stays in the record; nothing is expanded
        elif all(r[1] == 1 for r in mine):
            state.status[b] = 1 if state.cost[b] >= 0 else 0
        else:
            state.status[b] = -1
            for r in mine:
                if r[1] == -1:
                    new += children(r[6], 0 if b in whole else give)
        records += [tuple(r) for r in mine]
        nxt += len(new)
        if nxt > MAX_CUBES:
            raise ValueError("more than 2^22 cubes")
        state.paths[b] = new
    return records, first


def drop_spent(state, total):
    """the driver's total budget (exact.nearest_rounds): an instance whose work has reached ``total`` (an int, or one per instance) leaves
    the frontier; its status stays -1 and it keeps its cost and model.  Returns the instances dropped."""
    out = []
    for b, p in enumerate(state.paths):
        if p and state.work[b] >= (total if np.isscalar(total) else total[b]):
            state.paths[b] = []
            out.append(b)
    return out


def run(instances, hints=None, penalties=None, start=None, budget=0, give=0, whole=(), max_rounds=1 << 20, total=None):
    "rounds until the frontier is empty (``total``: with drop_spent after every round): the final State"
    state = State(instances, hints, penalties, start)
    for _ in range(max_rounds):
        if not state.cubes():
            break
        round(instances, state, budget, give, whole)
        if total is not None:
            drop_spent(state, total)
    return state
