"""Batches that make one wave of the complete solvers run instance after instance (a plain module like exact_wide.py), shared by
test_exact_reuse_host.py and test_exact_reuse_gpu.py, with the Python models' results on them.  Every result is computed once per process
(functools.lru_cache) and must not be modified by a test.

The three persistent kernels of csrc/pdp_exact.hip (k_exact, k_exact_learn, k_exact_check) launch min(B, CUs * resident workgroups)
workgroups of one wave; a wave takes instance after instance from one counter, in the host's launch order (``launch_order``), and runs
every LDS-routed one in the same slab as the one before.  The init of an instance clears val, pend, cnt (and req) only; trail, mark, dvar,
lev, rsn and the arena keep what the predecessor left, and since the layout's offsets depend on n, m, e and the arena, the successor's
arrays lie over other arrays of the predecessor.  With PDP_EXACT_GRID=1 the whole batch runs through one wave, so the batches here decide
what a successor finds:
  crossing()   literal counts strictly fall while variable counts strictly rise (variables without an occurrence, as padded() of
               test_exact_wide_gpu.py): every 4-byte array of a successor is longer than the predecessor's, so it starts over bytes where the
               predecessor kept literals, offsets and values (``overlaid``)
  shrinking()  the same clauses without the padding: the ordinary case, both counts fall
  routes()     HBM-routed instances (PAD_N variables: past the slab in all three layouts) and LDS-routed ones in one batch: one wave runs
               the HBM arrays first and the slab after
  tiled(B)     64 distinct tiny instances repeated to B: more than twice the natural grid of an MI355X with no switch set"""
import functools

import numpy as np

import exact_learn_model as lm
import exact_model
import exact_proof_model as pm
import exact_wide as xw
import families

LDS_LIMIT = 48 * 1024
PAD_N = 10000                # variables that put any instance past the slab of every layout (the checker's takes 5 bytes per variable)
CROSS_N0 = 12                # variables of crossing()'s first instance
CROSS_ARENA = 8              # the reduced arena of crossing(): two learned clauses of three literals fill it
CROSS_BUDGET = 30000         # clause-literal reads: some searches of crossing() end undecided
MIXED_BUDGET = 20000         # of the plain search on the mixed batch: chronological backtracking does not finish the larger thrash instances
ROUTES_BUDGET = 50000
ROUTES_ARENA = 40


# ---- the slab layouts of csrc/pdp_exact.hip, restated (test_exact_wide_gpu.plain_slab_bytes, test_exact_learn_gpu.slab_bytes and
# test_exact_proof_gpu.check_on_lds state the totals) ---------------------------------------------------------------------------------------
def per_variable_bytes(layout, n):
    """the bytes of the per-variable 4-byte arrays, which all three layouts put first: pend, cnt [2n], trail, mark [n+1], dvar [n+1] of
    ex_lds_layout; pend, cnt [2n], req [2n], trail, mark [n+1], lev, rsn of exl_lds_layout; req of exc_lds_layout.  The literals start here."""
    return {'plain': 20 * n + 8, 'learn': 36 * n + 4, 'check': 4 * n}[layout]


def slab_end(layout, n, m, e, arena=0):
    "the first byte past lit, the arena (learning layout: A = arena or 4 e u16 words), cptr [m+1] and val [n]"
    words = e + ((arena if arena else 4 * e) if layout == 'learn' else 0)
    return per_variable_bytes(layout, n) + 2 * words + 2 * (m + 1) + n


def overlaid(layout, pred, succ, arena=0):
    """The arithmetic the crossing batch rests on.  pred, succ = (n, m, e) of two instances that one wave runs one after the other, with
    n' > n and e' < e.  The successor's 4-byte arrays take per_variable_bytes(n') > per_variable_bytes(n) bytes from offset 0, so their
    tail covers [per_variable_bytes(n), ...): the bytes where the predecessor kept its literals and, if the tail is long enough, its arena,
    offsets and value bytes.  Returns the number of bytes of the successor's 4-byte arrays that lie over the predecessor's lit .. val."""
    (n, m, e), (n2, _, _) = pred, succ
    lo, hi = per_variable_bytes(layout, n), min(per_variable_bytes(layout, n2), slab_end(layout, n, m, e, arena))
    return max(0, hi - lo)


def dims(inst):
    "(n, m, e) of every instance, n as the library counts it"
    return [(n, len(c), int(e)) for n, (_, c), e in zip(xw.sizes(inst), inst, xw.edges(inst))]


def launch_order(inst, fits):
    """ex_prepare / exl_prepare / exc_prepare restated: the instances that do not fit the slab (HBM route) first, then the others, each
    group by literal count descending, ties by index.  ``fits``: instance -> bool."""
    e = xw.edges(inst)
    key = lambda i: (-int(e[i]), i)
    return sorted([i for i, x in enumerate(inst) if not fits(x)], key=key) + sorted([i for i, x in enumerate(inst) if fits(x)], key=key)


# ---- crossing() and shrinking() ------------------------------------------------------------------------------------------------------------
def uniform(n, m, seed):
    "uniform 3-SAT: m clauses on three distinct variables of n"
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(m):
        vs = rng.choice(n, size=3, replace=False) + 1
        out.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
    return n, out


@functools.lru_cache(maxsize=None)
def cores():
    """the clause sets of crossing() and shrinking(), literal counts strictly falling: uniform 3-SAT at 3.6 to 4.8 clauses per variable on 12,
    10 and 8 variables, and between them the family instances of as few literals (a regular one, a minimal one, thrash 12, 8 and 2)"""
    fam = {name: (n, c) for name, n, c in families.exact_cases()}
    picked = [fam['regular-4-2-n40'], fam['minimal-5'], lm.thrash(12), lm.thrash(8), fam['minimal-4'], lm.thrash(2)]
    unif = [uniform(12, m, 9000 + m) for m in range(56, 44, -1)] + [uniform(10, m, 9000 + m) for m in range(44, 35, -1)] + \
           [uniform(8, m, 9000 + m) for m in range(35, 29, -1)]
    out, seen = [], set()
    for inst, e in sorted(zip(picked + unif, xw.edges(picked + unif).tolist()), key=lambda t: -t[1]):        # stable: a family instance wins a tie
        if e not in seen:
            seen.add(e)
            out.append(inst)
    return out


def shrinking():
    return cores()


@functools.lru_cache(maxsize=None)
def cross_step():
    "(variables of the last instance of crossing(), the step between two instances): the last slab of the learning layout is within one step of 48 KiB"
    c = cores()
    _, m, e = dims(c)[-1]
    last = (LDS_LIMIT - (4 + 2 * 5 * e + 2 * (m + 1))) // 37                         # arena 0 (4 e words) is the larger arena of the small instances
    step = (last - CROSS_N0) // (len(c) - 1)
    return CROSS_N0 + step * (len(c) - 1), step


@functools.lru_cache(maxsize=None)
def crossing():
    _, step = cross_step()
    out = [(CROSS_N0 + k * step, c) for k, (n, c) in enumerate(cores())]
    assert all(a[0] >= b[0] for a, b in zip(out, cores()))
    return out


@functools.lru_cache(maxsize=None)
def cross_hints():
    """hints of shrinking() in the manner of 'nan30': a third of the instances gets the plain model's own assignment (every variable hinted:
    the check pass answers the satisfiable ones), a third random 0 / 1 for every variable (the check pass fails, the search follows), a third
    random 0 / 1 with 30 % NaN (no check pass)"""
    rng = np.random.RandomState(65)
    own = cross_plain(False)[0][1]
    out = []
    for i, n in enumerate(xw.sizes(cores())):
        h = rng.randint(0, 2, size=n).astype(np.float32)
        if i % 3 == 0:
            h = own[i].copy()
        elif i % 3 == 2:
            h[rng.rand(n) < 0.3] = np.nan
            h[0] = np.nan
        out.append(h)
    return out


def padded_hints(hints, inst):
    "xw.pad_hints with a size per instance"
    return [xw.pad_hints([h], n)[0] for h, n in zip(hints, xw.sizes(inst))]


@functools.lru_cache(maxsize=None)
def cross_plain(hinted):
    "(results, stats) of the plain model on shrinking(); crossing() differs by variables without an occurrence"
    return xw.plain_model(cores(), CROSS_BUDGET, cross_hints() if hinted else None)


@functools.lru_cache(maxsize=None)
def cross_learn(arena, hinted=False):
    return xw.learn_model(cores(), arena, CROSS_BUDGET, cross_hints() if hinted else None)


@functools.lru_cache(maxsize=None)
def cross_proof(arena):
    return pm.solve(cores(), budget=CROSS_BUDGET, arena=arena)


# ---- the mixed batch of test_exact_learn_gpu.py ------------------------------------------------------------------------------------------
def mixed():
    "small_instances() + family() + thrashes(): (instances, arena -> pm.solve of them), the cache of exact_proof_model"
    return pm.base_inputs()


@functools.lru_cache(maxsize=None)
def mixed_hints():
    "kind -> hints of the mixed batch, as xw.plain_hints()"
    inst = mixed()[0]
    rng = np.random.RandomState(66)
    nan30 = []
    for n in xw.sizes(inst):
        h = rng.randint(0, 2, size=n).astype(np.float32)
        h[rng.rand(n) < 0.3] = np.nan
        nan30.append(h)
    return {'own': [m.copy() for m in mixed_plain(None)[0][1]], 'nan30': nan30}


@functools.lru_cache(maxsize=None)
def mixed_plain(kind):
    return xw.plain_model(mixed()[0], MIXED_BUDGET, None if kind is None else mixed_hints()[kind])


# ---- routes() ----------------------------------------------------------------------------------------------------------------------------
ROUTES_HBM = (1, 2, 4, 7, 8, 29, 425, 432, 452, 461, 466, 470)                       # of the mixed batch: small ones, an empty clause, families, thrashes
ROUTES_LDS = tuple(range(10, 28)) + (59, 423, 430, 436, 440, 455, 462, 465, 468, 472)


def _routes_index():
    "(index into the mixed batch, over PAD_N variables?) of every instance of routes(): the two groups alternate"
    out = []
    for k in range(max(len(ROUTES_HBM), len(ROUTES_LDS))):
        out += [(i, True) for i in ROUTES_HBM[k:k + 1]] + [(i, False) for i in ROUTES_LDS[k:k + 1]]
    return out


def routes_cores():
    "routes() without the padding: what the models run on"
    inst = mixed()[0]
    return [inst[i] for i, _ in _routes_index()]


@functools.lru_cache(maxsize=None)
def routes():
    """(instances, the same all padded to PAD_N): instances of the mixed batch, those of ROUTES_HBM over PAD_N variables.  In the batch the
    two groups alternate, so the launch order is the host's sort and not the order of the batch."""
    cores = routes_cores()
    return [(PAD_N, c) if big else (n, c) for (n, c), (_, big) in zip(cores, _routes_index())], [(PAD_N, c) for _, c in cores]


@functools.lru_cache(maxsize=None)
def routes_hints():
    inst = routes_cores()
    rng = np.random.RandomState(67)
    nan30 = []
    for n in xw.sizes(inst):
        h = rng.randint(0, 2, size=n).astype(np.float32)
        h[rng.rand(n) < 0.3] = np.nan
        nan30.append(h)
    return {'own': [m.copy() for m in routes_plain(None)[0][1]], 'nan30': nan30}


@functools.lru_cache(maxsize=None)
def routes_plain(kind):
    return xw.plain_model(routes_cores(), ROUTES_BUDGET, None if kind is None else routes_hints()[kind])


@functools.lru_cache(maxsize=None)
def routes_learn(arena, kind=None):
    return xw.learn_model(routes_cores(), arena, ROUTES_BUDGET, None if kind is None else routes_hints()[kind])


@functools.lru_cache(maxsize=None)
def routes_proof(arena):
    return pm.solve(routes_cores(), budget=ROUTES_BUDGET, arena=arena)


# ---- tiled(B) ----------------------------------------------------------------------------------------------------------------------------
TINY = 64


@functools.lru_cache(maxsize=None)
def tiny():
    "64 distinct instances of 3 to 8 variables and 4 to 30 clauses of 1 to 3 literals"
    rng = np.random.RandomState(68)
    out = []
    while len(out) < TINY:
        n = int(rng.randint(3, 9))
        m = int(rng.randint(4, min(30, 5 * n) + 1))
        clauses = []
        for _ in range(m):
            k = int(rng.choice([1, 2, 3], p=[0.05, 0.25, 0.7]))
            vs = rng.choice(n, size=k, replace=False) + 1
            clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=k))])
        if (n, clauses) not in out:
            out.append((n, clauses))
    return out


@functools.lru_cache(maxsize=None)
def tiled_index(B):
    "which tiny instance stands at each of the B positions: every one about B / 64 times, in a fixed shuffled order"
    idx = np.arange(B) % TINY
    np.random.RandomState(69).shuffle(idx)
    return idx


def tiled(B):
    t = tiny()
    return [t[i] for i in tiled_index(B)]


@functools.lru_cache(maxsize=None)
def tiny_results():
    "the models on tiny(): dict of the plain search's three outputs, pm.solve's seven and pm.check_all's three on what pm.solve answered"
    t = tiny()
    proof = pm.solve(t)
    regions = [pm.words(x) for x in proof[5]]
    return dict(plain=exact_model.solve(t), proof=proof, regions=regions, check=pm.check_all(t, proof[0], proof[1], regions, proof[6]))


# ---- what a predecessor can be --------------------------------------------------------------------------------------------------------------
def predecessors(order, flags):
    "how many instances with ``flags`` true are followed by another one in launch order (under grid 1: run before another in the same wave)"
    return int(sum(bool(flags[i]) for i in order[:-1]))
