"""The resumable counting search (pdp_exact_count_round / pdp_exact_count_expand, include/pdp_hip.h) stated in plain Python.

A cube is a *path*: a list of (bit, closed) pairs, one per decision level from level 1 on.  (0, 0) is a level on the polarity the search
tries first whose other polarity is still owed, (0, 1) the first polarity with nothing owed, (1, 1) the other polarity; (1, 0) is refused.
The root cube is the empty path.  ``cube`` is tests/exact_count_model.py's search with the decisions of the path's levels taken from the
path, a budget that is tested only where a node begins and that does not charge the replay of the path, and, at a budget stop, the
checkpoint: the path of the open levels at that moment.  ``expand`` re-cuts the checkpoints of a round into the next round's frontier,
``round`` runs a whole frontier and adds what it counted to the running totals in cube order.  All the arithmetic is IEEE double in
exactly the order written here, and csrc/pdp_exact.hip does the same operations in the same order.  Slow: meant for small instances."""
import math

import numpy as np

MAX_N = 1023                    # as exact_count_model.MAX_N
ROUND_BUDGET = 1 << 18         # PDP_EXACT_ROUND_BUDGET: the reads per cube and round when budget <= 0
MAX_CUBES = 1 << 22


def check_path(n, path):
    "the refusals of one path: its length and the (1, 0) pair"
    if not 0 <= len(path) <= n:
        raise ValueError("a path of %d levels on %d variables" % (len(path), n))
    for L, (bit, closed) in enumerate(path, 1):
        if bit and not closed:
            raise ValueError("level %d is (1, 0)" % L)


def cube(n, clauses, path, budget):
    """(status 1 / -1, count float, true_count float64 [n], work, leaves, replay, checkpoint) of one cube.  ``replay`` is the reads made
    before the budget began to count, ``checkpoint`` the path to resume from (status -1) or None (status 1)."""
    if budget <= 0:
        budget = ROUND_BUDGET
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    assert n <= MAX_N
    check_path(n, path)
    work, leaves, count = 0, 0, 0.0
    T, F = [0.0] * n, [0.0] * n
    snap = {0: 0.0}
    val = [0] * n
    trail, mark, dvar, other = [], {0: 0}, {}, {}
    level, plen, base, fresh = 0, len(path), None, True

    def credit(lv):
        "the models counted since level lv was opened go to the variables on its part of the trail"
        d = count - snap[lv]
        for u in trail[mark[lv]:]:
            if val[u] == 1:
                T[u] += d
            else:
                F[u] += d

    status = 1
    while True:
        if fresh:
            # a node begins: the first one with level >= plen starts the budget's clock, every one tests it
            if base is None and level >= plen:
                base = work
            if base is not None and work - base >= budget:
                status = -1
                break
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
        if not conflict and pend:
            continue
        if not conflict and wmin is None:
            # a leaf.  Inside the path (level < plen) it is counted iff every remaining path bit of levels level+1 .. plen is 0; either
            # way the search backtracks as after a conflict
            if level >= plen or all(path[L - 1][0] == 0 for L in range(level + 1, plen + 1)):
                count = count + math.ldexp(1.0, n - len(trail))
                leaves += 1
            conflict = True
        if conflict:
            resumed = False
            while level > 0:
                v, second = dvar[level]
                first = val[v]
                credit(level)
                for u in trail[mark[level]:]:
                    val[u] = 0
                del trail[mark[level]:]
                if not second:
                    dvar[level] = (v, True)
                    other[level] = 1
                    val[v] = 3 - first
                    trail.append(v)
                    snap[level] = count
                    resumed = True
                    break
                level -= 1
            if not resumed:
                break
            plen = min(plen, level)                                               # the path beyond a flipped level no longer applies
            fresh = True
            continue
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
        level += 1
        bit, closed = path[level - 1] if level <= plen else (0, 0)
        if bit:
            positive = not positive
        mark[level] = len(trail)
        dvar[level] = (v, bool(closed))
        other[level] = int(bit)
        snap[level] = count
        val[v] = 1 if positive else 2
        trail.append(v)
        fresh = True
    checkpoint = [(other[L], int(dvar[L][1])) for L in range(1, level + 1)] if status == -1 else None
    # the end (out of levels, or out of budget): every open level is flushed, the newest first, level 0 with mark 0
    while level >= 0:
        credit(level)
        del trail[mark[level]:]
        level -= 1
    true_count = np.asarray([T[v] + (count - T[v] - F[v]) * 0.5 for v in range(n)], dtype=np.float64)
    return status, count, true_count, work, leaves, (work if base is None else base), checkpoint


def children(checkpoint, give):
    "the cubes a stopped cube becomes: a child per given level, shallowest first, then the remainder with those levels closed"
    owed = [L for L, (_, closed) in enumerate(checkpoint, 1) if not closed][:max(give, 0)]
    out = [[(b, 1) for b, _ in checkpoint[:L - 1]] + [(1, 1)] for L in owed]
    out.append([(b, 1 if L in owed else c) for L, (b, c) in enumerate(checkpoint, 1)])
    return out


def inst_n(inst):
    n, clauses = inst
    return max([n] + [abs(int(l)) for c in clauses for l in c if int(l) != 0])


class State:
    """The running totals and the open frontier of a batch: ``paths[b]`` the open cubes of instance b in cube order, ``count`` [B],
    ``true_count`` a list of float64 arrays, ``work`` / ``leaves`` [B], ``rounds`` [B] the rounds instance b had a cube in."""

    def __init__(self, instances):
        self.n = [inst_n(i) for i in instances]
        self.paths = [[[]] if n <= MAX_N else [] for n in self.n]
        self.count = [0.0] * len(instances)
        self.true_count = [np.zeros(n, dtype=np.float64) for n in self.n]
        self.work = [0] * len(instances)
        self.leaves = [0] * len(instances)
        self.rounds = [0] * len(instances)

    def status(self):
        return [-2 if n > MAX_N else (-1 if p else 1) for n, p in zip(self.n, self.paths)]

    def cubes(self):
        return sum(len(p) for p in self.paths)


def round(instances, state, budget=0, give=0, whole=()):
    """One round: every open cube runs for ``budget`` reads past its replay, the totals take what it counted in cube order, and the
    frontier becomes the expansion of the checkpoints.  ``whole``: the instances that are never expanded (the HBM route's).  Returns
    the per-cube records [(instance, status, count, work, leaves, replay, checkpoint)] in cube order."""
    records = []
    nxt = 0
    for b, (n, clauses) in enumerate(instances):
        new = []
        if state.paths[b]:
            state.rounds[b] += 1
        for path in state.paths[b]:
            st, c, tc, w, lv, replay, cp = cube(n, clauses, path, budget)
            records.append((b, st, c, w, lv, replay, cp))
            state.count[b] = state.count[b] + c
            for v in range(len(tc)):
                state.true_count[b][v] = state.true_count[b][v] + tc[v]
            state.work[b] += w
            state.leaves[b] += lv
            if st == -1:
                new += children(cp, 0 if b in whole else give)
        nxt += len(new)
        if nxt > MAX_CUBES:
            raise ValueError("more than 2^22 cubes")
        state.paths[b] = new
    return records


def run(instances, budget=0, give=0, whole=(), max_rounds=1 << 20):
    "rounds until the frontier is empty: the final State"
    state = State(instances)
    for _ in range(max_rounds):
        if not state.cubes():
            break
        round(instances, state, budget, give, whole)
    return state


def words(n_max):
    "words per path row (pdp_exact_count_frontier_words)"
    return max(1, (n_max + 31) // 32)


def pack(paths, W):
    "(len int32 [C], bits int32 [C, W], closed int32 [C, W]) of a list of paths: level L is bit (L - 1) % 32 of word (L - 1) // 32"
    C = len(paths)
    ln = np.zeros(C, dtype=np.int32)
    bits = np.zeros((C, W), dtype=np.uint32)
    closed = np.zeros((C, W), dtype=np.uint32)
    for c, path in enumerate(paths):
        ln[c] = len(path)
        for i, (b, cl) in enumerate(path):
            bits[c, i >> 5] |= np.uint32(int(b) << (i & 31))
            closed[c, i >> 5] |= np.uint32(int(cl) << (i & 31))
    return ln, bits.view(np.int32), closed.view(np.int32)


def unpack(ln, bits, closed):
    "the inverse of pack"
    bits, closed = np.asarray(bits).view(np.uint32), np.asarray(closed).view(np.uint32)
    return [[(int(bits[c, i >> 5] >> (i & 31)) & 1, int(closed[c, i >> 5] >> (i & 31)) & 1) for i in range(int(ln[c]))]
            for c in range(len(ln))]


def frontier(state, W):
    "(cube_off int64 [B+1], len, bits, closed) of a State's open cubes"
    off = np.zeros(len(state.paths) + 1, dtype=np.int64)
    flat = []
    for b, p in enumerate(state.paths):
        off[b + 1] = off[b] + len(p)
        flat += p
    return (off,) + pack(flat, W)
