"""The split weighted counting search (pdp_exact_mass_split, include/pdp_hip.h) stated in plain Python: one instance's solution mass,
posterior and open mass from 2^depth cubes.

A cube is tests/exact_mass_model.py's search with the decisions of levels 1..depth pinned by the bits of the cube's index, exactly as in
tests/exact_count_split_model.py (the most significant of the ``depth`` bits belongs to level 1; 0 = the polarity the mass search tries
first -- the heavier literal, at exactly 0.5 the count's rule --, 1 = the other one; a pinned level counts as already flipped, so
backtracking pops through it and the open mass leaves its other half to the sibling cube).  Three more rules:
  * a pinned decision whose product ``mass * w(pinned literal)`` is 0.0 is a conflict at once, without a pass (exact_mass_model's flip
    rule: a pinned "other" polarity is a flip);
  * a leaf met with fewer than ``depth`` levels open is reached by every cube that shares those levels' bits and is credited to the one
    whose remaining bits are all 0 (exact_count_split_model's rule);
  * when the budget fires with fewer than ``depth`` levels open, every cube that shares those levels' bits stands at the same node after
    the same reads: the node's mass goes into the open mass of the one whose remaining bits are all 0.
All the arithmetic is IEEE double in exactly the order written here -- per cube as in exact_mass_model.py, then over the cubes in
ascending index -- and csrc/pdp_exact.hip does the same operations in the same order.  With weights that are multiples of 1/8 and
n <= 17 every product and sum is exact.  Slow: every cube replays its prefix; meant for instances of up to about 30 variables."""
import numpy as np

from exact_mass_model import MAX_N, chunk_product
from exact_model import NO_BUDGET

MAX_DEPTH = 16


def _weights(n, clauses, weights):
    "(clauses without zeros, n, the weights as float32, refusal 0 / -2 / -3)"
    cl = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in cl for l in c])
    w32 = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert w32.size == n, (w32.size, n)
    if n > MAX_N:
        return cl, n, w32, -2
    if not bool(((w32 >= 0) & (w32 <= 1)).all()):                                 # a NaN fails both comparisons
        return cl, n, w32, -3
    return cl, n, w32, 0


def cube(n, clauses, weights, budget, depth, index):
    """(status 1 / -1, mass float, true_mass float64 [n], open_mass float, work, leaves) of cube ``index`` of the 2^depth cubes.  The
    budget is the cube's own: ``work >= budget`` before every pass, on the cube's own reads."""
    if budget <= 0:
        budget = 1 << 32
    assert 0 <= depth <= MAX_DEPTH and 0 <= index < (1 << depth)
    cl, n, w32, refused = _weights(n, clauses, weights)
    assert not refused
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in cl]              # (variable, the value that makes the literal true)
    p = [float(x) for x in w32]

    def omega(v, x):
        return p[v] if x == 1 else 1.0 - p[v]

    def owns(lv):
        "the cube owns a node met with lv levels open: outside the prefix, or its remaining bits are 0"
        return lv >= depth or index & ((1 << (depth - lv)) - 1) == 0

    work, leaves, Z, mass = 0, 0, 0.0, 1.0
    T, F = [0.0] * n, [0.0] * n
    snap, pre = {0: 0.0}, {}
    val = [0] * n
    trail, mark, dvar = [], {0: 0}, {}
    level = 0

    def credit(lv):
        "the mass counted since level lv was opened goes to the variables on its part of the trail"
        d = Z - snap[lv]
        for u in trail[mark[lv]:]:
            if val[u] == 1:
                T[u] += d
            else:
                F[u] += d

    status = 1
    dead = False                    # a pinned decision of mass 0.0: a conflict at once, without a pass and without a budget check
    while True:
        conflict = dead
        if not dead:
            if work >= budget:
                status = -1
                break
            # one unit-propagation pass
            pend, wmin = {}, None
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
            old = len(trail)
            for v in sorted(pend):
                val[v] = 1 if pend[v] & 1 else 2
                conflict = conflict or pend[v] == 3
                trail.append(v)
            # the pass's new entries, 64 consecutive ones at a time, ascending
            for base in range(old, len(trail), 64):
                mass = mass * chunk_product([omega(u, val[u]) for u in trail[base:base + 64]])
            if mass == 0.0:
                conflict = True
            if not conflict and pend:
                continue
            if not conflict and wmin is None:
                # a leaf.  Inside the prefix (level < depth) every cube with these levels' bits arrives here: the one whose remaining
                # bits are 0 takes it, the others add nothing; either way the search backtracks as after a conflict
                if owns(level):
                    Z = Z + mass
                    leaves += 1
                conflict = True
        dead = False
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
                    val[v] = 3 - first
                    trail.append(v)
                    snap[level] = Z
                    mass = pre[level] * omega(v, val[v])
                    if mass == 0.0:
                        continue        # the other half has no mass: a conflict at once, without a pass (the level is undone next)
                    resumed = True
                    break
                level -= 1
            if not resumed:
                break
            continue
        # branching: the count's variable; the heavier literal first, the count's polarity at exactly 0.5
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
        if p[v] > 0.5:
            positive = True
        elif p[v] < 0.5:
            positive = False
        else:
            positive = cnt.get((v, 1), 0) >= cnt.get((v, 2), 0)
        level += 1
        pinned = level <= depth
        if pinned and (index >> (depth - level)) & 1:                             # the cube's bit of this level: the other polarity
            positive = not positive
        mark[level] = len(trail)
        dvar[level] = (v, pinned)                                                 # a pinned level is never flipped
        pre[level] = mass
        snap[level] = Z
        val[v] = 1 if positive else 2
        trail.append(v)
        mass = mass * omega(v, val[v])
        dead = pinned and mass == 0.0
    # the mass not yet visited: the untried halves of the open levels, oldest first (a pinned level's other half is the sibling cube's),
    # then the current node where the cube owns it
    open_mass = 0.0
    if status == -1:
        for lv in range(1, level + 1):
            v, second = dvar[lv]
            if not second:
                open_mass = open_mass + pre[lv] * omega(v, 3 - val[v])
        if owns(level):
            open_mass = open_mass + mass
    # the end (out of levels, or out of budget): every open level is flushed, the newest first, level 0 with mark 0
    while level >= 0:
        credit(level)
        del trail[mark[level]:]
        level -= 1
    true_mass = np.asarray([T[v] + (Z - T[v] - F[v]) * p[v] for v in range(n)], dtype=np.float64)
    return status, Z, true_mass, open_mass, work, leaves


def search(n, clauses, weights, budget=NO_BUDGET, depth=0):
    """(status, mass, true_mass float64 [n], open_mass, work, leaves, depth_used, cubes) of the instance from its 2^depth cubes, summed in
    ascending index: status 1 if every cube's is 1, else -1 (Z then lies in [mass, mass + open_mass]); cubes = [(status, mass, open_mass,
    work, leaves)].  n > 1023: status -2, depth_used 0, every other output 0 and the one record (-2, 0.0, 0.0, 0, 0), at every depth.  A
    weight that is NaN or outside [0, 1]: status -3, every other output 0, depth_used the depth asked for and the record (-3, 0.0, 0.0,
    0, 0) for each of its cubes."""
    cl, n, w32, refused = _weights(n, clauses, weights)
    if refused == -2:
        return -2, 0.0, np.zeros(n, dtype=np.float64), 0.0, 0, 0, 0, [(-2, 0.0, 0.0, 0, 0)]
    if refused == -3:
        return -3, 0.0, np.zeros(n, dtype=np.float64), 0.0, 0, 0, depth, [(-3, 0.0, 0.0, 0, 0)] * (1 << depth)
    mass, open_mass, work, leaves = 0.0, 0.0, 0, 0
    true_mass = np.zeros(n, dtype=np.float64)
    cubes = []
    for j in range(1 << depth):
        st, z, tm, op, w, lv = cube(n, cl, w32, budget, depth, j)
        cubes.append((st, z, op, w, lv))
        mass = mass + z
        open_mass = open_mass + op
        for v in range(n):
            true_mass[v] = true_mass[v] + tm[v]
        work += w
        leaves += lv
    status = 1 if all(c[0] == 1 for c in cubes) else -1
    return status, mass, true_mass, open_mass, work, leaves, depth, cubes


def solve(instances, weights, budget=NO_BUDGET, depths=0):
    "search() over a list (depths: an int or one per instance): a list of its tuples"
    if isinstance(depths, int):
        depths = [depths] * len(instances)
    return [search(n, c, w, budget, d) for (n, c), w, d in zip(instances, weights, depths)]
