"""Instances, hints, depths and references shared by test_exact_min_unsat_split_host.py and test_exact_min_unsat_split_gpu.py
(pdp_exact_min_unsat_split)."""
import functools

import numpy as np

import exact_min_unsat_cases as cs
import exact_min_unsat_model as mm
import exact_min_unsat_split_model as sm

KINDS = cs.KINDS
RATIOS = (4.26, 5.0, 6.0)


@functools.lru_cache(maxsize=None)
def family():
    "125 instances of at most 12 variables (the degenerate ones included) and the three kinds of hints for them"
    return cs.family(35, 116, 12)


@functools.lru_cache(maxsize=None)
def family_brute():
    return [cs.brute_min(n, c) for n, c in family()[0]]


def uniform_3sat(seed, n, per_ratio):
    rng = np.random.RandomState(seed)
    return [cs.threshold_3sat(rng, n, int(round(n * r))) for r in RATIOS for _ in range(per_ratio)]


@functools.lru_cache(maxsize=None)
def batch():
    """(instances, hints per kind, depths): the family plus uniform 3-SAT of n = 20 (three per ratio) and n = 30 (one per ratio) at
    clause ratios 4.26 / 5.0 / 6.0, depths mixed over 0..6.  Every instance finishes at the default budget on the model, at its depth
    and under each kind of hints."""
    few, kinds = family()
    more = uniform_3sat(20, 20, 3) + uniform_3sat(30, 30, 1)
    rng = np.random.RandomState(12)
    extra = {k: cs.hints_of(rng, more, k) for k in KINDS}
    inst = few + more
    depth = np.random.RandomState(7).randint(0, 7, size=len(inst)).astype(np.int8)
    depth[len(few):] = np.resize(np.arange(1, 7), len(more))                       # every large instance is split, over all depths
    return inst, {k: kinds[k] + extra[k] for k in KINDS}, depth


@functools.lru_cache(maxsize=None)
def batch_plain(kind):
    "exact_min_unsat_model.solve on the batch"
    inst, hints, _ = batch()
    return mm.solve(inst, hints[kind])


@functools.lru_cache(maxsize=None)
def batch_sequential(kind):
    "the split model's sequential() on the batch at its depths, computed once"
    inst, hints, depth = batch()
    return sm.solve(inst, hints[kind], depths=depth.tolist())


def prefix_only():
    """n = 3 cannot open eight levels: every leaf lies inside the prefix.  The block costs every assignment exactly one clause, the two
    other clauses are satisfiable with it: optimum 1; the all-false hint leaves 2 unsatisfied"""
    return 3, cs.block(1, 2, 3) + [[1, 2], [-1, 3]]
