"""The specification of the complete search under assumptions (tests/exact_assume_model.py; pdp_exact_solve_learn_assume in
include/pdp_hip.h) on the CPU: without assumptions it is the learning model (A1), against enumeration its status, models and failed sets
are right (A2-A5), the backbone it defines is the enumerated one, and the constructed instances reach what they are built for -- level 1
opened again after a backjump to level 0, the singleton failure at an opening, an opening and a final analysis past one wave's width, a
reduction while a level-1 variable rests on a learned clause.  test_exact_assume_gpu.py runs the kernel on the same instances."""
import functools
import os

import numpy as np

import exact_assume_model as am
import exact_learn_model as lm
import families
from helpers import REPO
from test_exact_learn_host import satisfies

RATIOS = (3.0, 4.26, 5.5)
SMALL_ARENA = 40
REDUCED_SEEDS, REDUCED_ARENA = (4000, 4008, 4019), 24


@functools.lru_cache(maxsize=None)
def random_family(per_ratio=80, seed=911):
    "random 3-SAT, 6 <= n <= 12, at the three ratios, each with 0 .. n random assumptions: ([(n, clauses)], [int8 assumptions])"
    rng = np.random.RandomState(seed)
    inst, assume = [], []
    for ratio in RATIOS:
        for _ in range(per_ratio):
            n = int(rng.randint(6, 13))
            clauses = []
            for _ in range(int(round(ratio * n))):
                vs = rng.choice(n, size=3, replace=False) + 1
                clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
            a = np.zeros(n, dtype=np.int8)
            k = int(rng.randint(0, n + 1))
            a[rng.choice(n, size=k, replace=False)] = rng.choice([-1, 1], size=k)
            inst.append((n, clauses))
            assume.append(a)
    return inst, assume


@functools.lru_cache(maxsize=None)
def random_results(arena=0):
    "(am.solve's six outputs, the statistics) of random_family() at one arena"
    inst, assume = random_family()
    stats = []
    return am.solve(inst, assume=assume, arena=arena, stats=stats), stats


def reopened(k=4):
    "(a) thrash(k) with the first variable of every binary clause assumed false: the last three variables are refuted above level 1"
    n, clauses = lm.thrash(k)
    a = np.zeros(n, dtype=np.int8)
    a[0:2 * k:2] = -1
    return (n, clauses), a


def against_level0(L=12):
    "(b) unit_chain(L) makes every variable true at level 0; variables L - 4 and L - 1 are assumed false, variable 2 true"
    a = np.zeros(L, dtype=np.int8)
    a[L - 5], a[L - 2], a[1] = -1, -1, 1
    return families.unit_chain(L), a


def wide_opening(n=130, k=80, seed=5):
    "(c) a planted 3-SAT instance on 130 variables with 80 of them assumed at the planted value, spread over all three chunks of ids"
    rng = np.random.RandomState(seed)
    planted = rng.randint(0, 2, size=n)
    clauses = []
    while len(clauses) < 3 * n:
        vs = rng.choice(n, size=3, replace=False)
        sg = rng.choice([-1, 1], size=3)
        if any((sg[j] > 0) == bool(planted[vs[j]]) for j in range(3)):
            clauses.append([int(v + 1) * int(s) for v, s in zip(vs, sg)])
    a = np.zeros(n, dtype=np.int8)
    pick = rng.choice(n, size=k, replace=False)
    a[pick] = np.where(planted[pick] > 0, 1, -1)
    return (n, clauses), a


def wide_final(K=70, s=3):
    """(d) a_j -> b_j for j = 1 .. K, all b_j together imply z, z implies y and not y; the a_j are assumed.  Level 1 takes three passes
    and ends in a conflict; the final analysis resolves with z's reason of K + 1 literals, walks 2 K + 2 trail slots and blames all K
    assumptions.  Strided, so that their ids lie in several chunks of 64."""
    A = lambda j: j
    Bv = lambda j: K + j
    z, y = 2 * K + 1, 2 * K + 2
    clauses = [[-A(j), Bv(j)] for j in range(1, K + 1)] + [[-Bv(j) for j in range(1, K + 1)] + [z], [-z, y], [-z, -y]]
    n, clauses = families.stride((2 * K + 2, clauses), s)
    a = np.zeros(n, dtype=np.int8)
    a[[(A(j) - 1) * s for j in range(1, K + 1)]] = 1
    return (n, clauses), a


def reduced(seed):
    """(e) threshold 3-SAT on 19 to 24 variables with one to three assumptions; at REDUCED_ARENA words the seeds of REDUCED_SEEDS reduce the
    arena while a level-1 variable rests on a learned clause (a lemma that a backjump to level 1 made unit there)"""
    rng = np.random.RandomState(seed)
    n = int(rng.randint(19, 25))
    clauses = []
    for _ in range(int(round(4.26 * n))):
        vs = rng.choice(n, size=3, replace=False) + 1
        clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
    a = np.zeros(n, dtype=np.int8)
    k = int(rng.randint(1, 4))
    a[rng.choice(n, size=k, replace=False)] = rng.choice([-1, 1], size=k)
    return (n, clauses), a


@functools.lru_cache(maxsize=None)
def constructed():
    "name -> ((n, clauses), assumptions, arena)"
    out = {'reopened': reopened() + (0,), 'against-level-0': against_level0() + (0,), 'wide-opening': wide_opening() + (0,),
           'wide-final': wide_final() + (0,)}
    for seed in REDUCED_SEEDS:
        out['reduced-%d' % seed] = reduced(seed) + (REDUCED_ARENA,)
    return out


@functools.lru_cache(maxsize=None)
def constructed_results():
    "name -> (am.search's six outputs, the statistics)"
    out = {}
    for name, ((n, clauses), a, arena) in constructed().items():
        st = {}
        out[name] = (am.search(n, clauses, None, a, arena=arena, stats=st), st)
    return out


def same_search(got, want):
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and tuple(got[2:5]) == tuple(want[2:5])


def agrees(model, a):
    return all((model[v] > 0.5) == (a[v] > 0) for v in np.nonzero(a)[0])


# ---- A1 ------------------------------------------------------------------------------------------------------------------------------------
def test_without_assumptions_it_is_the_learning_search():
    inst = [(n, c) for _, n, c in families.exact_cases()] + [lm.thrash(k) for k in range(2, 13)]
    for arena in (0, 12, 40):
        for n, c in inst:
            want = lm.search(n, c, arena=arena)
            for a in (None, np.zeros(max([n] + [abs(l) for x in c for l in x]), dtype=np.int8)):
                got = am.search(n, c, None, a, arena=arena)
                same_search(got, want)
                assert got[5].size == 0
    # and with hints: the check pass and the polarities are the learning model's
    rng = np.random.RandomState(3)
    for n, c in random_family()[0][:60]:
        h = rng.randint(0, 2, size=n).astype(np.float32)
        h[rng.rand(n) < 0.2] = np.nan
        same_search(am.search(n, c, h, None), lm.search(n, c, h))


# ---- A2 - A5 against enumeration -----------------------------------------------------------------------------------------------------------
def test_status_model_and_failed_set_against_enumeration():
    inst, assume = random_family()
    assert len(inst) >= 200
    for arena in (0, SMALL_ARENA):
        (status, models, work, learned, reductions, failed), _ = random_results(arena)
        seen = {1: 0, 0: 0, 'failed': 0, 'alone': 0}
        for (n, c), a, s, m, f in zip(inst, assume, status, models, failed):
            if s == -1:
                assert arena and f.size == 0
                continue
            assert (len(am.brute(*am.units(n, c, a))) > 0) == (s == 1)                                          # A4
            seen[int(s)] += 1
            if s == 1:
                assert satisfies(c, m) and agrees(m, a) and f.size == 0                                         # A2
            else:
                assert not m.any() and set(f.tolist()) <= set(np.nonzero(a)[0].tolist())                        # A3
                assert len(am.brute(*am.units(n, c, a, only=f))) == 0
                seen['failed'] += f.size > 0
                seen['alone'] += f.size == 0
        if arena == 0:
            assert (status != -1).all()
        assert min(seen.values()) >= 10, seen


def test_a_model_as_the_assumptions_is_accepted_by_the_check_pass():
    inst, _ = random_family()
    base = am.solve(inst)
    sat = [i for i in range(len(inst)) if base[0][i] == 1]
    assert len(sat) >= 60
    for i in sat[:60]:
        n, c = inst[i]
        a = np.where(base[1][i] > 0.5, 1, -1).astype(np.int8)
        contrary = 1.0 - base[1][i]                                                                            # hints against every assumption
        for h in (None, contrary):
            got = am.search(n, c, h, a)
            assert got[0] == 1 and np.array_equal(got[1], base[1][i]) and got[2] == am.check_reads(c, base[1][i])[0] and got[3] == 0   # A5


def test_a_contradicted_hint_is_overridden():
    inst, assume = random_family()
    rng = np.random.RandomState(8)
    n_sat = 0
    for (n, c), a in list(zip(inst, assume))[:90]:
        h = np.where(a > 0, 0.0, 1.0).astype(np.float32)                # against every assumption, "true first" elsewhere
        h[rng.rand(n) < 0.3] = np.nan
        got = am.search(n, c, h, a)
        assert got[0] == am.search(n, c, None, a)[0]
        if got[0] == 1:
            n_sat += 1
            assert satisfies(c, got[1]) and agrees(got[1], a)
    assert n_sat >= 15


# ---- the backbone --------------------------------------------------------------------------------------------------------------------------
def test_backbone_is_the_enumerated_one():
    inst, _ = random_family()
    forced = free = 0
    for n, c in inst[::2]:
        models = am.brute(n, c)
        st, bb = am.backbone(n, c)
        assert (st == 1) == (len(models) > 0)
        if st != 1:
            assert bb is None
            continue
        want = np.where(models.all(axis=0), 1, np.where((~models).all(axis=0), -1, 0)).astype(np.int8)
        np.testing.assert_array_equal(bb, want)
        forced += int((want != 0).sum())
        free += int((want == 0).sum())
    assert forced > 50 and free > 50
    # a budget that ends the base search: no backbone, and never a wrong +-1
    n, c = next((n, c) for n, c in inst if am.search(n, c)[0] == 1)
    assert am.backbone(n, c, budget=1) == (-1, None)


# ---- the constructed cases -----------------------------------------------------------------------------------------------------------------
def test_level_one_is_opened_again_after_a_backjump_to_level_zero():
    (out, st), ((n, c), a, _) = constructed_results()['reopened'], constructed()['reopened']
    assert st['opens'] >= 2 and out[0] == 0 and out[3] >= 2
    assert out[5].size == 0 and len(am.brute(n, c)) == 0                 # refuted at level 0 in the end: unsatisfiable on its own


def test_singleton_failure_at_the_opening():
    (out, st), ((n, c), a, _) = constructed_results()['against-level-0'], constructed()['against-level-0']
    assert out[0] == 0 and out[5].tolist() == [n - 5] and st['opens'] == 1 and st['failed'] == 1 and 'final_span' not in st
    assert out[2] == lm.search(n, c)[2] and out[3] == 0                  # the opening reads nothing: the reads are the level-0 passes'


def test_an_opening_past_one_wave():
    (out, st), ((n, c), a, _) = constructed_results()['wide-opening'], constructed()['wide-opening']
    assert n == 130 and st['assumed'] >= 70 and out[0] == 1 and satisfies(c, out[1]) and agrees(out[1], a)
    assert len({int(v) // 64 for v in np.nonzero(a)[0]}) == 3


def test_a_final_analysis_past_one_wave():
    (out, st), ((n, c), a, _) = constructed_results()['wide-final'], constructed()['wide-final']
    assert out[0] == 0 and st['final_span'] > 64 and st['final_len'] > 64 and st['failed'] > 64 and st['assumed'] > 64
    np.testing.assert_array_equal(out[5], np.nonzero(a)[0])
    assert len({int(v) // 64 for v in out[5]}) > 1
    assert out[3] == 0                                                   # nothing is learned from the final analysis


def test_a_reduction_while_level_one_rests_on_learned_clauses():
    names = [k for k in constructed() if k.startswith('reduced-')]
    assert len(names) == 3
    for k in names:
        out, st = constructed_results()[k]
        assert st['live_l1'] > 0 and out[4] > 0 and out[0] == 0 and out[5].size > 0 and st['final_span'] > 0


# ---- header and symbol ---------------------------------------------------------------------------------------------------------------------
def test_header_and_symbol():
    from pdp import native
    header = open(os.path.join(REPO, 'include', 'pdp_hip.h')).read()
    proto = ("int pdp_exact_solve_learn_assume(pdp_problem *p, const float *hint, const int8_t *assume, int64_t budget, int64_t arena,\n"
             "                                 int8_t *status, float *model, int64_t *work, int32_t *learned, int8_t *failed, void *stream);")
    assert proto in header and '#define PDP_ABI_VERSION 3' in header
    assert all(('A%d ' % k) in header for k in range(1, 6))
    assert 'pdp_exact_solve_learn_assume' in native.EXPORTED_SYMBOLS
    assert hasattr(native.Problem, 'exact_solve_assume')
