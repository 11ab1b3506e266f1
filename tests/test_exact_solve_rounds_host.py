"""The resumable deciding search without a GPU: its Python statement (tests/exact_solve_rounds_model.py) run until the frontier is empty
against brute force and the plain deciding search's (tests/exact_model.py), for budgets and gives that stop it at every node, without
hints, with random hints and with hints that hold NaNs; the progress rule and the work bound on every round; the give = 0 identity;
caller-made frontiers of closed paths, which meet a model inside a path; dropped cubes; a copied state; the refusals; the header."""
import copy
import functools
import importlib
import itertools
import os
import re
import sys

import numpy as np
import pytest

import exact_count_cases as cs
import exact_model as em
import exact_solve_rounds_model as sm
from helpers import REPO

PAIRS = [(1, 0), (1, 3), (40, 1), (200, 8)]            # reads per cube and round, levels given away per stopped cube
KINDS = ('none', 'random', 'nan')


def hints_of(inst, kind, seed=5):
    "per instance None, or an array of inst_n values in [0, 1]; 'nan': about a third of them NaN"
    if kind == 'none':
        return None
    rng = np.random.RandomState(seed)
    out = []
    for i in inst:
        h = rng.rand(sm.inst_n(i)).astype(np.float32)
        if kind == 'nan':
            h[rng.rand(len(h)) < 0.35] = np.nan
        out.append(h)
    return out


@functools.lru_cache(maxsize=None)
def plain(kind):
    fam, hints = cs.family(), hints_of(cs.family(), kind)
    return [em.search(n, c, None if hints is None else hints[b]) for b, (n, c) in enumerate(fam)]


def satisfies(clauses, model):
    return all(any((model[abs(l) - 1] > 0.5) == (l > 0) for l in c if l != 0) for c in clauses)


def accepted(n, clauses, hints):
    "(the plain call's check pass runs and accepts, its reads when it runs)"
    code = em.hint_codes(n, hints)
    if not all(code):
        return False, 0
    reads, ok = em.check_reads([[int(l) for l in c if int(l) != 0] for c in clauses], [1.0 if c == 1 else 0.0 for c in code])
    return ok, reads


def node_bound(n, clauses):
    "the reads of one node: at most n + 1 propagation passes of at most e reads each, and a branching pass of at most 2 e"
    e = sum(len(c) for c in clauses)
    return (n + 3) * e


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('budget,give', PAIRS)
def test_rounds_decide_as_the_plain_search(budget, give, kind):
    fam, brute, want = cs.family(), cs.family_brute(), plain(kind)
    hints = hints_of(fam, kind)
    assert len(fam) >= 400
    state = sm.State(fam, hints)
    rounds, dropped, fresh_work = 0, 0, [0] * len(fam)
    while state.cubes():
        before = [list(p) for p in state.paths]
        rec, first = sm.round(fam, state, budget, give)
        rounds += 1
        flat = [(b, p) for b, ps in enumerate(before) for p in ps]
        assert len(rec) == len(flat)
        for (b0, path), (b, st, work, replay, cp) in zip(flat, rec):
            n, clauses = fam[b]
            assert b == b0 and st in (1, 0, -1, sm.DROPPED)
            assert (st in (1, 0)) == (cp == []) and (st in (1, 0) or cp != path)  # no round returns its checkpoint unchanged
            assert replay <= work <= replay + budget + node_bound(sm.inst_n(fam[b]), clauses)
            assert st in (1, 0) or work - replay >= budget
            sm.check_path(sm.inst_n(fam[b]), cp)
            fresh_work[b] += work - replay
        for b in range(len(fam)):
            mine = [r for r in rec if r[0] == b]
            ones = [j for j, r in enumerate(mine) if r[1] == 1]
            assert first[b] == (ones[0] if ones else -1)
            if ones:
                # a decided instance leaves the frontier: its stopped cubes are dropped and nothing of them is expanded
                assert state.status[b] == 1 and state.paths[b] == [] and all(r[1] != -1 for r in mine)
                dropped += sum(r[1] == sm.DROPPED for r in mine)
            else:
                assert all(r[1] != sm.DROPPED for r in mine)
                assert state.status[b] == (-1 if state.paths[b] else (0 if mine else state.status[b]))
    for b, (n, clauses) in enumerate(fam):
        assert state.status[b] == (1 if brute[b][0] > 0 else 0) == want[b][0], b
        assert state.model[b].dtype == np.float32 and len(state.model[b]) == sm.inst_n(fam[b])
        if state.status[b] == 1:
            assert satisfies(clauses, state.model[b]), b
        else:
            assert not state.model[b].any()
        if give == 0:
            # one cube throughout: the plain search interrupted and resumed
            ok, reads = accepted(sm.inst_n(fam[b]), clauses, state.hint(b))
            if not ok:
                np.testing.assert_array_equal(state.model[b], want[b][1])
                assert fresh_work[b] + reads == want[b][2], b                     # the replay is the only extra work
    assert rounds == max(state.rounds) and rounds >= 3                            # the family has trees of several nodes
    assert (dropped > 0) == (give > 0)
    print('%s hints, budget %d give %d: %d rounds, %d cubes dropped, reads %.2f times the plain search'
          % (kind, budget, give, rounds, dropped, sum(state.work) / max(1, sum(w[2] for w in want))))


@pytest.mark.parametrize('n,ratio,budget,give', [(20, 4.3, 3000, 0), (20, 4.3, 3000, 4), (30, 4.3, 5000, 0), (30, 5.0, 3000, 8)])
def test_uniform_3sat(n, ratio, budget, give):
    inst = cs.uniform_3sat(n + give, n, (ratio,), 3)
    hints = hints_of(inst, 'nan', seed=n)
    state = sm.run(inst, hints, budget, give)
    for b, (k, c) in enumerate(inst):
        w = em.search(k, c, hints[b])
        assert state.status[b] == w[0] and (w[0] == 0 or satisfies(c, state.model[b]))
        if give == 0:
            np.testing.assert_array_equal(state.model[b], w[1])
    assert max(state.rounds) > 1


def finish(n, clauses, hints, paths, budget, give):
    "(satisfiable?, the models met) of a caller-made frontier, run until it is empty or a cube answers 1"
    models = []
    while paths:
        nxt = []
        for p in paths:
            st, model, _, _, cp = sm.cube(n, clauses, hints, p, budget)
            if st == 1:
                models.append(model)
            elif st == -1:
                nxt += sm.children(cp, give)
        if models:
            break
        paths = nxt
    return bool(models), models


@pytest.mark.parametrize('depth', [1, 2, 3, 4, 5])
def test_closed_paths_of_every_depth_decide_as_the_instance(depth):
    # 2^depth paths of closed levels are pdp_exact_solve_split's cubes: where the tree is shallower than the path, a model is met inside
    # the path, by every cube that shares its levels' bits, and each of them answers 1 with it
    fam, brute = cs.family()[::4], cs.family_brute()[::4]
    hints = hints_of(fam, 'nan')
    inside = 0
    for b, ((n, c), br) in enumerate(zip(fam, brute)):
        n = sm.inst_n((n, c))
        if depth > n:
            continue
        paths = [[(x, 1) for x in bits] for bits in itertools.product((0, 1), repeat=depth)]
        for budget, give in ((1 << 30, 0), (60, 1)):
            sat, models = finish(n, c, hints[b], paths, budget, give)
            assert sat == (br[0] > 0) and all(satisfies(c, m) for m in models)
        whole = [sm.cube(n, c, hints[b], p, 1 << 30) for p in paths]
        assert all(w[0] in (0, 1) and w[4] is None for w in whole)
        shared = len(set(w[1].tobytes() for w in whole if w[0] == 1)) < sum(w[0] == 1 for w in whole)
        inside += shared
    assert inside > 10


def test_open_levels_of_a_caller_made_path():
    # (0, 0) on every level is the root cube met later: the same answer and model; the two closed halves of level 1 hold all the models
    inst = [i for i in cs.uniform_3sat(5, 16, (3.0,), 4)]
    for n, clauses in inst:
        w = em.search(n, clauses)
        root = sm.cube(n, clauses, None, [(0, 0)] * 3, 1 << 30)
        assert root[0] == w[0] and np.array_equal(root[1], w[1])
        half, other = sm.cube(n, clauses, None, [(0, 1)], 1 << 30), sm.cube(n, clauses, None, [(1, 1)], 1 << 30)
        assert max(half[0], other[0]) == w[0]
        if half[0] == 1:
            assert np.array_equal(half[1], w[1])                                  # the plain search's first model lies in the first half


def test_a_copied_state_finishes_the_same():
    fam = cs.family()[:150] + cs.uniform_3sat(9, 20, (4.3,), 4)
    hints = hints_of(fam, 'random')
    state = sm.State(fam, hints)
    for _ in range(3):
        sm.round(fam, state, 40, 1)
    assert state.cubes() > 0
    held = copy.deepcopy(state)
    while state.cubes():
        sm.round(fam, state, 40, 1)
    while held.cubes():
        sm.round(fam, held, 40, 1)
    assert held.status == state.status and held.work == state.work and held.rounds == state.rounds
    assert all(np.array_equal(a, b) for a, b in zip(held.model, state.model))
    # other budgets and gives from the copy on: the same statuses, models that satisfy
    again = sm.State(fam, hints)
    for r in range(1 << 20):
        if not again.cubes():
            break
        sm.round(fam, again, 40 if r < 3 else 500, 1 if r < 3 else 3)
    assert again.status == state.status
    assert all(satisfies(c, m) for (n, c), m, s in zip(fam, again.model, again.status) if s == 1)


def test_refusals():
    n, clauses = 4, [[1, 2], [-1, 3], [2, -4]]
    for path in ([(1, 0)], [(0, 1), (1, 0)], [(0, 0)] * 5):
        with pytest.raises(ValueError):
            sm.cube(n, clauses, None, path, 10)
    wide = (1024, [[1, 2], [-1, 1024]])
    state = sm.State([(n, clauses), wide])
    assert state.paths == [[[]], []] and state.status == [-1, -2]
    done = sm.run([(n, clauses), wide], None, 5, 1)
    assert done.status == [1, -2] and done.work[1] == 0 and done.rounds[1] == 0 and not done.model[1].any()
    assert sm.cube(n, clauses, None, [], 0)[0] == 1                               # budget <= 0: the default, far above this tree
    with pytest.raises(AssertionError):
        sm.cube(n, clauses, [0.5] * 3, [], 10)                                    # one hint per variable


def test_header_and_symbols():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    m = re.search(r'#define PDP_EXACT_SOLVE_ROUND_BUDGET \(\(\(int64_t\)1\) << (\d+)\)', text)
    assert '#define PDP_ABI_VERSION 3' in text and m
    assert ("int pdp_exact_solve_round(pdp_problem *p, const float *hint, const int64_t *cube_off, int64_t cubes, const int32_t *len, "
            "const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status, float *model, int64_t *work, int32_t *first, "
            "int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out, int64_t *cube_work, int64_t *cube_replay, "
            "void *stream);") in text
    from pdp import exact, native
    assert 'pdp_exact_solve_round' in native.EXPORTED_SYMBOLS
    assert exact.SOLVE_ROUND_BUDGET == sm.ROUND_BUDGET == 1 << int(m.group(1))
    assert ['cube_off', 'len', 'bits', 'closed', 'hint', 'status', 'model', 'work', 'rounds'] == list(native.SolveState.FIELDS)
    assert hasattr(native.Problem, 'exact_solve_begin') and hasattr(native.Problem, 'exact_solve_round') and hasattr(exact, 'solve_rounds')


@pytest.mark.parametrize('kw', [dict(split='rounds', round_budget=0), dict(split='rounds', rounds=-1), dict(split='rounds', round_budget=1.5),
                                dict(split=3, rounds=2), dict(round_budget=5), dict(split='auto', round_budget=5)])
def test_solve_items_refuses_bad_rounds(kw):
    from pdp import exact
    with pytest.raises(ValueError, match='round'):
        exact.solve_items([exact.raw_item(2, [[1, 2]])], **kw)


@pytest.mark.parametrize('kw', [dict(learn=True), dict(certify=True), dict(assume=[np.array([1, 0])])])
def test_rounds_spread_the_plain_search_only(kw):
    from pdp import exact
    with pytest.raises(ValueError, match='without learn, certify and assume'):
        exact.solve_items([exact.raw_item(2, [[1, 2]])], split='rounds', **kw)


def test_the_other_searches_keep_refusing_rounds():
    from pdp import exact
    item = [exact.raw_item(2, [[1, 2]])]
    for call in (lambda: exact.min_unsat(item, split='rounds'), lambda: exact.nearest_model(item, [np.zeros(2, dtype=np.float32)], split='rounds'),
                 lambda: exact.solution_mass(item, [np.full(2, 0.5, dtype=np.float32)], split='rounds')):
        with pytest.raises(ValueError, match='split must be'):
            call()


@pytest.mark.parametrize('argv,said', [(['--complete-rounds', '3'], 'give --complete as well'),
                                       (['--complete', '--complete-rounds', '41'], 'from 0 to 40'),
                                       (['--complete', '--complete-rounds', '-2'], 'from 0 to 40'),
                                       (['--complete', '--complete-rounds', '3', '--complete-split', '2'], 'without --complete-split'),
                                       (['--complete', '--complete-rounds', '3', '--complete-learn'], 'without --complete-learn'),
                                       (['--complete', '--complete-rounds', '3', '--complete-certify'],
                                        'without --complete-learn and --complete-certify')])
def test_command_line_refusals(argv, said, capsys):
    # parser errors: they end the command before a file is opened or a GPU is asked for
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    try:
        satyr = importlib.import_module('satyr')
    finally:
        sys.path.pop(0)
    yaml = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
    with pytest.raises(SystemExit) as e:
        satyr.main([yaml, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d'] + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and '--complete-rounds' in err and said in err
