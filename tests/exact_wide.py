"""Instances past one wave's width for the complete solvers (a plain module like families.py), shared by test_exact_wide_host.py and
test_exact_wide_gpu.py: the batches, and the Python models' results on them with the models' statistics.  Every result is computed once
per process (functools.lru_cache) and must not be modified by a test.

One wave of 64 lanes runs an instance (csrc/pdp_exact.hip), so the code that differs past 64 is: the units of one pass assigned in chunks
of 64 variables, a level of more than 64 trail entries undone, the backwards trail scan of the analysis in windows of 64 slots, conflict,
reason and learned clauses of more than 64 literals, an arena reduction over more than 64 live clauses that keeps a clause with an old
index past 64 or one longer than 64 literals, and branch keys and hint codes of variables past the first chunk.  The families
(tests/families.py): fan -- a pass of 100 units at level 0 and trails past 128; wide / wide_kept -- clauses of D + 1 and D + 2 literals,
the latter with a reduction that keeps one of D; far_uip -- K trail slots between two variables of one analysis, and K + 4 entries undone
in one step; stride -- the same searches on variable ids spread over five times as many chunks."""
import functools

import numpy as np

import exact_learn_model as lm
import exact_model
import families
from test_exact_learn_host import small_instances

FAN_SEEDS, FAN_ARENA, FAN_BUDGET = (0, 1, 2, 4), 1500, 5_000_000        # fan(120, seed) for the learning search
PLAIN_SEEDS, PLAIN_BUDGET = (0, 1, 2, 3, 4, 5), 3_000_000               # fan(100, seed) for the plain and the hinted search
WIDE_D = (70, 100, 130)
FAR_K = (63, 64, 65, 100, 130)                                          # the analysis steps to its second window of trail slots from K = 64
STRIDE = 5
LEARN_PAD_N, PLAIN_PAD_N = 1500, 2400                                   # 37 and 21 bytes of slab per variable: past 48 KiB


def small_arena(D):
    """words that hold wide_kept(D)'s first two learned clauses (D + 1 and D literals: 2 D + 3 words) but not the third (D + 1 literals)
    as well: the reduction keeps the second, the reason of a_D, and drops the first"""
    return 3 * D + 4


def few():
    "nine small instances, three before, between and after the wide ones of every batch"
    s = small_instances()
    return s[:3], s[3:6], s[6:9]


def fans():
    return [families.fan(120, s) for s in FAN_SEEDS]


def interleave(wide, more):
    a, b, c = few()
    return a + wide + b + more + c


@functools.lru_cache(maxsize=None)
def learn_batches():
    "name -> (instances, arena, budget) of the learning search; every instance is on the LDS route"
    f = fans()
    far = [families.far_uip(K) for K in FAR_K]
    wides = [families.wide(D) for D in WIDE_D]
    kept = [families.wide_kept(D) for D in WIDE_D]
    out = {'fan': (interleave(f + far, [families.stride(f[0], STRIDE), families.stride(f[3], STRIDE)] + wides), FAN_ARENA, FAN_BUDGET),
           'wide-0': (interleave(wides + kept, [families.stride(families.wide(100), STRIDE), families.stride(families.wide_kept(100), STRIDE)] + far),
                      0, 0)}
    for D in WIDE_D:
        s = STRIDE if D <= 100 else 3                                   # wide(130) at stride 5 is past the LDS route
        out['wide-%d' % D] = (interleave([families.wide(D), families.wide_kept(D)],
                                         [families.stride(families.wide(D), s), families.stride(families.wide_kept(D), s)]), small_arena(D), 0)
    return out


@functools.lru_cache(maxsize=None)
def plain_batch():
    "the instances of the plain and the hinted search (budget PLAIN_BUDGET), all on the LDS route"
    f = [families.fan(100, s) for s in PLAIN_SEEDS]
    wides = [families.wide(D) for D in WIDE_D] + [families.wide_kept(D) for D in WIDE_D]
    return interleave(f + [families.far_uip(K) for K in FAR_K],
                      wides + [families.stride(f[0], STRIDE), families.stride(f[3], STRIDE), families.stride(families.wide(100), STRIDE)])


def sizes(inst):
    return [max([n] + [abs(l) for c in cl for l in c]) for n, cl in inst]


def edges(inst):
    return np.array([sum(len(c) for c in cl) for _, cl in inst], dtype=np.int64)


def learn_model(inst, arena, budget, hints=None):
    "(lm.solve's five outputs, the statistics of every instance)"
    stats = [{} for _ in inst]
    out = [lm.search(n, c, None if hints is None else hints[i], budget or exact_model.NO_BUDGET, arena, stats=stats[i]) for i, (n, c) in enumerate(inst)]
    return (np.array([o[0] for o in out], dtype=np.int8), [o[1] for o in out], np.array([o[2] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int32), np.array([o[4] for o in out], dtype=np.int32)), stats


def plain_model(inst, budget, hints=None):
    "(exact_model.solve's three outputs, the statistics of every instance)"
    stats = [{} for _ in inst]
    out = [exact_model.search(n, c, None if hints is None else hints[i], budget or exact_model.NO_BUDGET, stats=stats[i]) for i, (n, c) in enumerate(inst)]
    return (np.array([o[0] for o in out], dtype=np.int8), [o[1] for o in out], np.array([o[2] for o in out], dtype=np.int64)), stats


@functools.lru_cache(maxsize=None)
def learn_results(name):
    inst, arena, budget = learn_batches()[name]
    return learn_model(inst, arena, budget)


@functools.lru_cache(maxsize=None)
def plain_hints():
    """kind -> hints of plain_batch(): 'own' the plain model's assignment (the satisfying one where it found one, all false elsewhere),
    'nan30' random 0 / 1 with 30 % NaN"""
    inst = plain_batch()
    rng = np.random.RandomState(64)
    nan30 = []
    for n in sizes(inst):
        h = rng.randint(0, 2, size=n).astype(np.float32)
        h[rng.rand(n) < 0.3] = np.nan
        nan30.append(h)
    return {'own': [m.copy() for m in plain_results(None)[0][1]], 'nan30': nan30}


@functools.lru_cache(maxsize=None)
def plain_results(kind):
    "the plain model on plain_batch() under the hints of `kind` (None: without hints)"
    return plain_model(plain_batch(), PLAIN_BUDGET, None if kind is None else plain_hints()[kind])


@functools.lru_cache(maxsize=None)
def plain_learn_results(kind):
    "the learning model at the default arena on plain_batch() under the same hints"
    return learn_model(plain_batch(), 0, PLAIN_BUDGET, None if kind is None else plain_hints()[kind])


def peak(stats, key):
    return max(s.get(key, 0) for s in stats)


def pad_hints(hints, n):
    """hints of instances padded to n variables: NaN for the variables without an occurrence where the instance has a NaN already, false
    where every variable has a hint, so that the check pass runs for the same instances as without the padding"""
    return [np.concatenate([h, np.full(n - len(h), np.nan if np.isnan(h).any() else 0.0, dtype=np.float32)]) for h in hints]
