"""The resumable deciding search (pdp_exact_solve_round, then pdp_exact_count_expand; include/pdp_hip.h) stated in plain Python.

The frontier is tests/exact_count_rounds_model.py's, unchanged: a cube is a path of (bit, closed) pairs, one per decision level, and
``children``, ``pack``, ``unpack``, ``words`` and ``frontier`` are that module's.  ``cube`` is the deciding search of tests/exact_model.py
without its check pass, with the decisions of the path's levels taken from the path (bit 0: the polarity the search would try first, the
hint's where the variable has one; bit 1: the other), the round budget of the counting rounds -- tested only where a node begins, the
replay of the path free against it -- and, at a budget stop, the checkpoint.  A state without an open clause answers 1 wherever it is
met, also inside the path: every cube that reaches it holds the same model.  ``round`` runs a whole frontier: an instance takes the
model of its lowest cube that answered 1 and drops its stopped cubes (cube status -2, nothing of them is expanded), is unsatisfiable
when every cube answered 0, and stays open otherwise.  No cube reads a word of another, so every record is a function of the inputs.
Slow: meant for small instances."""
import numpy as np

from exact_count_rounds_model import MAX_CUBES, MAX_N, check_path, children, frontier, inst_n, pack, unpack, words  # noqa: F401
from exact_model import hint_codes

ROUND_BUDGET = 1 << 18         # PDP_EXACT_SOLVE_ROUND_BUDGET: the reads per cube and round when budget <= 0
DROPPED = -2                   # record of a stopped cube whose instance another cube of the round has answered


def cube(n, clauses, hints, path, budget):
    """(status 1 / 0 / -1, model float32 [n], work, replay, checkpoint) of one cube.  ``replay`` is the reads made before the budget began
    to count, ``checkpoint`` the path to resume from (status -1) or None."""
    if budget <= 0:
        budget = ROUND_BUDGET
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    assert n <= MAX_N
    check_path(n, path)
    code = hint_codes(n, hints)
    zeros = np.zeros(n, dtype=np.float32)
    work = 0
    val = [0] * n
    trail, mark, dvar, other = [], {}, {}, {}
    level, plen, base, fresh = 0, len(path), None, True

    def done(status, model, checkpoint=None):
        return status, model, work, (work if base is None else base), checkpoint

    while True:
        if fresh:
            # a node begins: the first one with level >= plen starts the budget's clock, every one tests it
            if base is None and level >= plen:
                base = work
            if base is not None and work - base >= budget:
                return done(-1, zeros, [(other[L], int(dvar[L][1])) for L in range(1, level + 1)])
            fresh = False
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
                    other[level] = 1
                    val[v] = 3 - first
                    trail.append(v)
                    resumed = True
                    break
                level -= 1
            if not resumed:
                return done(0, zeros)
            plen = min(plen, level)                                               # the path beyond a flipped level no longer applies
            fresh = True
            continue
        if pend:
            continue
        if wmin is None:
            # no open clause: a model, wherever it is met (inside the path too)
            return done(1, np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32))
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
        bit, closed = path[level - 1] if level <= plen else (0, 0)
        if bit:
            positive = not positive
        mark[level] = len(trail)
        dvar[level] = (v, bool(closed))
        other[level] = int(bit)
        val[v] = 1 if positive else 2
        trail.append(v)
        fresh = True


class State:
    """The answers and the open frontier of a batch: ``paths[b]`` the open cubes of instance b in cube order, ``status`` [B] (-1 open, 1,
    0, -2 not searched), ``model`` a list of float32 arrays (zeros until status 1), ``work`` [B], ``rounds`` [B] the rounds instance b had a
    cube in, ``hints`` a list of arrays or None."""

    def __init__(self, instances, hints=None):
        self.n = [inst_n(i) for i in instances]
        self.hints = hints
        self.paths = [[[]] if n <= MAX_N else [] for n in self.n]
        self.status = [-1 if n <= MAX_N else -2 for n in self.n]
        self.model = [np.zeros(n, dtype=np.float32) for n in self.n]
        self.work = [0] * len(instances)
        self.rounds = [0] * len(instances)

    def cubes(self):
        return sum(len(p) for p in self.paths)

    def hint(self, b):
        return None if self.hints is None else self.hints[b]


def round(instances, state, budget=0, give=0, whole=()):
    """One round: every open cube runs for ``budget`` reads past its replay; then the outcome of every instance that has cubes, and the
    frontier becomes the expansion of the cubes that are still stopped.  ``whole``: the instances that are never expanded (the HBM
    route's).  Returns (records [(instance, status, work, replay, checkpoint)] in cube order, first [B]: the lowest cube of the instance,
    counted from its own first one, that answered 1; -1: none, or no cube)."""
    records, first = [], [-1] * len(instances)
    nxt = 0
    for b, (n, clauses) in enumerate(instances):
        if not state.paths[b]:
            continue
        state.rounds[b] += 1
        mine = []
        for path in state.paths[b]:
            st, model, w, replay, cp = cube(n, clauses, state.hint(b), path, budget)
            state.work[b] += w
            if st == 1 and first[b] < 0:
                first[b] = len(mine)
                state.model[b] = model
            mine.append([b, st, w, replay, cp or []])
        new = []
        if first[b] >= 0:
            state.status[b] = 1
            for r in mine:
                if r[1] == -1:
                    r[1] = DROPPED                                                # its checkpoint stays in the record; nothing is expanded
        elif all(r[1] == 0 for r in mine):
            state.status[b] = 0
        else:
            for r in mine:
                if r[1] == -1:
                    new += children(r[4], 0 if b in whole else give)
        records += [tuple(r) for r in mine]
        nxt += len(new)
        if nxt > MAX_CUBES:
            raise ValueError("more than 2^22 cubes")
        state.paths[b] = new
    return records, first


def run(instances, hints=None, budget=0, give=0, whole=(), max_rounds=1 << 20):
    "rounds until the frontier is empty: the final State"
    state = State(instances, hints)
    for _ in range(max_rounds):
        if not state.cubes():
            break
        round(instances, state, budget, give, whole)
    return state
