"""Instances, depths, start models and references shared by test_exact_nearest_split_host.py and test_exact_nearest_split_gpu.py
(pdp_exact_nearest_split).  Every result is computed once per process (functools.lru_cache) and must not be modified by a test."""
import functools

import numpy as np

import exact_nearest_cases as nc
import exact_nearest_model as nm
import exact_nearest_split_model as sm

VARIANTS = ('mixed', 'unit', 'start')       # mixed penalties; no penalties (all 1); mixed penalties and a start model on every instance


@functools.lru_cache(maxsize=None)
def batch():
    "exact_nearest_cases.batch() without its n = 50 instances, a depth 0..6 per instance: (inst, hints, pens, depth int8)"
    inst, hints, pens = nc.batch()
    keep = [i for i, (n, _) in enumerate(inst) if n < 50]
    depth = np.random.RandomState(4500).randint(0, 7, size=len(keep)).astype(np.int8)
    return [inst[i] for i in keep], [hints[i] for i in keep], [pens[i] for i in keep], depth


@functools.lru_cache(maxsize=None)
def starts():
    """one assignment per instance of batch(): on every third instance a model by the plain deciding search (random bits where there is
    none), random bits elsewhere -- the kernel checks every one of them, and so does the statement"""
    inst = batch()[0]
    rng = np.random.RandomState(4600)
    out = []
    for i, (n, c) in enumerate(inst):
        m = nc.any_model(n, c) if i % 3 == 0 else None
        out.append(rng.randint(0, 2, size=n).astype(np.float32) if m is None else m.copy())
    return out


def dressed(variant):
    "(hints, pens, starts) of a variant of batch()"
    _, hints, pens, _ = batch()
    return hints, (None if variant == 'unit' else pens), (starts() if variant == 'start' else None)


@functools.lru_cache(maxsize=None)
def batch_sequential(variant):
    "the statement's sequential() on batch() at its depths"
    inst, _, _, depth = batch()
    hints, pens, begin = dressed(variant)
    return sm.solve(inst, hints, pens, begin, depths=depth.tolist())


@functools.lru_cache(maxsize=None)
def batch_plain(variant):
    "the plain statement on batch(): exact_nearest_model.solve's tuple"
    inst = batch()[0]
    hints, pens, _ = dressed(variant)
    return nm.solve(inst, hints, pens)


def attains(inst, hint, pen, res):
    """the model of a sequential() / interleaved() result satisfies every clause at its cost from the hint, and the cube that holds the
    cost says so; cost -1: no model, model all 0"""
    n, clauses = inst
    status, cost, model, work, improvements, first, start_cost, cubes = res
    assert model.dtype == np.float32
    if cost < 0:
        assert first == -1 and not model.any() and status in (0, -1)
        return
    bits = nm.threshold(len(model), hint)
    assert nc.satisfies(clauses, model) and nm.distance(bits, nm.penalty_list(len(model), pen), model) == cost
    assert first == -1 or cubes[first][2] == cost
    assert first >= 0 or cost in (0, start_cost)
    assert all(c[2] == sm.NO_COST or c[2] >= cost for c in cubes)
    assert improvements == sum(c[3] for c in cubes) and (first >= 0) == any(c[2] == cost for c in cubes)
    assert start_cost < 0 or cost <= start_cost


def prefix_only():
    "n = 3: every leaf lies inside a prefix of 8 levels"
    return 3, [[1, 2], [-1, 3], [-2, -3], [1, 3]]
