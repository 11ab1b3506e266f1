"""The resumable nearest-model search without a GPU: its Python statement (tests/exact_nearest_rounds_model.py) run until the frontier is
empty against brute force and the plain branch and bound's (tests/exact_nearest_model.py), for budgets and gives that stop it at every
node, with the Hamming distance and with mixed penalties; the promises R2 (one cube: the plain call), R3 (any give: its status and cost),
R4 (the cost is attained and never rises) and R5 (bounded progress) on every cube of every round; caller-made frontiers of closed paths,
which meet leaves and pinned flips inside a path; start models; a copied state; the refusals; the header."""
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
import exact_nearest_cases as nc
import exact_nearest_model as nm
import exact_nearest_rounds_model as rm
from exact_min_unsat_model import threshold
from helpers import REPO

PAIRS = [(1, 0), (1, 3), (40, 1), (200, 8)]            # reads per cube and round, levels given away per stopped cube


@functools.lru_cache(maxsize=None)
def plain(mixed):
    inst, hints, pens = nc.small()
    return [nm.search(n, c, hints[b], pens[b] if mixed else None) for b, (n, c) in enumerate(inst)]


def check_pass(n, clauses, hints):
    "(the plain call's check pass accepts the hint, its reads)"
    bits = threshold(n, hints)
    reads, ok = 0, True
    for c in clauses:
        c = [int(l) for l in c if int(l) != 0]
        k = next((j + 1 for j, l in enumerate(c) if (l > 0) == bool(bits[abs(l) - 1])), None)
        reads += len(c) if k is None else k
        ok = ok and k is not None
    return ok, reads


def node_bound(n, clauses):
    "the reads of one node: at most n + 1 propagation passes of at most e reads each, and a branching pass of at most 2 e"
    return (n + 3) * sum(len(c) for c in clauses)


def attained(inst, state, b):
    "R4: cost -1 with a model of zeros, or a model of the instance at exactly that penalty distance"
    n, clauses = inst[b]
    n = rm.inst_n(inst[b])
    if state.cost[b] < 0:
        return not state.model[b].any()
    return (nc.satisfies(clauses, state.model[b])
            and nm.distance(threshold(n, state.hint(b)), nm.penalty_list(n, state.pen(b)), state.model[b]) == state.cost[b])


def checked_round(inst, state, budget, give):
    "one round of the model with R4 and R5 asserted on every cube and instance: (records, first)"
    before = [list(p) for p in state.paths]
    cost_in = list(state.cost)
    rec, first = rm.round(inst, state, budget, give)
    flat = [(b, p) for b, ps in enumerate(before) for p in ps]
    assert len(rec) == len(flat)
    for (b0, path), (b, st, cc, work, replay, imp, cp) in zip(flat, rec):
        assert b == b0 and st in (1, -1, rm.DROPPED)
        assert (st == 1) == (cp == []) and (st == 1 or cp != path)                # R5: no round returns its checkpoint unchanged
        assert replay <= work <= replay + budget + node_bound(rm.inst_n(inst[b]), inst[b][1])
        assert st == 1 or work - replay >= budget
        assert (cc >= 0) == (imp > 0) and (cost_in[b] < 0 or cc < cost_in[b])     # a cube accepts below the bound it was given only
        rm.check_path(rm.inst_n(inst[b]), cp)
    for b in range(len(inst)):
        mine = [r for r in rec if r[0] == b]
        if not mine:
            assert first[b] == -1 and state.cost[b] == cost_in[b]
            continue
        found = [r[2] for r in mine if r[2] >= 0]
        assert state.cost[b] == (min(found) if found else cost_in[b])
        assert first[b] == (next(j for j, r in enumerate(mine) if r[2] == state.cost[b]) if found else -1)
        assert cost_in[b] < 0 or state.cost[b] <= cost_in[b]                      # R4: it never rises
        assert attained(inst, state, b)
        stopped = any(r[1] == -1 for r in mine)
        if state.cost[b] == 0:
            assert state.status[b] == 1 and state.paths[b] == [] and not stopped
        else:
            assert all(r[1] != rm.DROPPED for r in mine)
            assert state.status[b] == (-1 if stopped else (1 if state.cost[b] >= 0 else 0)) and bool(state.paths[b]) == stopped
    return rec, first


@pytest.mark.parametrize('mixed', [False, True])
@pytest.mark.parametrize('budget,give', PAIRS)
def test_rounds_find_the_plain_minimum(budget, give, mixed):
    inst, hints, pens = nc.small()
    want = plain(mixed)
    assert len(inst) >= 400
    state = rm.State(inst, hints, pens if mixed else None)
    rounds, dropped, fresh = 0, 0, [0] * len(inst)
    while state.cubes():
        rec, _ = checked_round(inst, state, budget, give)
        rounds += 1
        dropped += sum(r[1] == rm.DROPPED for r in rec)
        for r in rec:
            fresh[r[0]] += r[3] - r[4]
    unsat = 0
    for b, (n, clauses) in enumerate(inst):
        n = rm.inst_n(inst[b])
        least = nc.brute(n, clauses, threshold(n, hints[b]), nm.penalty_list(n, pens[b] if mixed else None))[0]
        assert (state.status[b], state.cost[b]) == (want[b][0], want[b][1]) == ((1, least) if least is not None else (0, -1)), b   # R3
        assert state.model[b].dtype == np.float32 and len(state.model[b]) == n and attained(inst, state, b)
        unsat += least is None
        if give == 0:
            # R2, one cube throughout: the plain search interrupted and resumed
            ok, reads = check_pass(n, clauses, hints[b])
            np.testing.assert_array_equal(state.model[b], want[b][2])
            if ok:
                # the plain call stops at its check pass; the rounds follow the hint to the same model and count that leaf
                assert (state.cost[b], state.improvements[b], want[b][4]) == (0, 1, 0)
                np.testing.assert_array_equal(state.model[b], np.asarray(threshold(n, hints[b]), dtype=np.float32))
            else:
                assert state.improvements[b] == want[b][4] and fresh[b] + reads == want[b][3], b
    assert rounds == max(state.rounds) and rounds >= 3 and 4 * unsat >= len(inst)
    print('mixed %s, budget %d give %d: %d rounds, %d cubes dropped, reads %.2f times the plain search'
          % (mixed, budget, give, rounds, dropped, sum(state.work) / max(1, sum(w[3] for w in want))))


@pytest.mark.parametrize('n', [20, 30])
def test_one_cube_is_the_plain_search_on_uniform_3sat(n):
    inst = cs.uniform_3sat(5200 + n, n, (3.5, 4.0, 4.5), 2)
    hints, pens = nc.dress(inst, 4200)
    state = rm.run(inst, hints, pens, None, 3000, 0)
    for b, (k, c) in enumerate(inst):
        w = nm.search(k, c, hints[b], pens[b])
        ok, reads = check_pass(k, c, hints[b])
        assert (state.status[b], state.cost[b]) == w[:2] and np.array_equal(state.model[b], w[2])
        assert ok or state.improvements[b] == w[4]
    assert max(state.rounds) > 3
    # R3 with the bound exchanged between many cubes
    for budget, give in ((200, 8), (3000, 2)):
        shared = rm.run(inst, hints, pens, None, budget, give)
        assert shared.status == state.status and shared.cost == state.cost
        assert all(attained(inst, shared, b) for b in range(len(inst)))


@pytest.mark.parametrize('depth', [1, 2, 3, 4, 5])
def test_closed_paths_of_every_depth_hold_the_minimum(depth):
    # 2^depth paths of closed levels are pdp_exact_nearest_split's cubes.  Where the tree is shallower than the path a leaf is met inside
    # the path, by every cube that shares its levels' bits; a bit-1 level whose penalty reaches the bound is pruned before any pass
    inst, hints, pens = nc.small()
    inside = at_once = 0
    for b in range(0, len(inst), 4):
        n, c = rm.inst_n(inst[b]), inst[b][1]
        if depth > n:
            continue
        w = nm.search(n, c, hints[b], pens[b])
        paths = [[(x, 1) for x in bits] for bits in itertools.product((0, 1), repeat=depth)]
        whole = [rm.cube(n, c, hints[b], pens[b], p, 1 << 30, None) for p in paths]
        assert all(r[0] == 1 and r[6] is None and (r[1] >= 0) == (r[5] > 0) for r in whole)
        found = [r[1] for r in whole if r[1] >= 0]
        assert (min(found) if found else -1) == w[1]
        inside += len(set(r[2].tobytes() for r in whole if r[1] >= 0)) < len(found)
        # the same frontier through the rounds, the bound exchanged: the plain status and cost, an attained model
        for budget, give in ((1 << 30, 0), (60, 1)):
            state = rm.State([inst[b]], [hints[b]], [pens[b]])
            state.paths[0] = [list(p) for p in paths]
            while state.cubes():
                checked_round([inst[b]], state, budget, give)
            assert (state.status[0], state.cost[0]) == w[:2]
        if w[1] > 0:
            # under the optimum as the bound nothing is accepted, and a path against a heavy variable ends without a pass
            tight = [rm.cube(n, c, hints[b], pens[b], p, 1 << 30, w[1]) for p in paths]
            assert all(r[0] == 1 and r[1] == -1 and r[5] == 0 for r in tight)
            at_once += any(r[3] < f[3] for r, f in zip(tight, whole))
    assert inside > 10 and at_once > 10


def test_open_levels_of_a_caller_made_path():
    # (0, 0) on every level is the root cube met later: the plain search; the two closed halves of level 1 hold the minimum between them
    inst = cs.uniform_3sat(5, 16, (3.0,), 4)
    hints, pens = nc.dress(inst, 7)
    for b, (n, clauses) in enumerate(inst):
        w = nm.search(n, clauses, hints[b], pens[b])
        root = rm.cube(n, clauses, hints[b], pens[b], [(0, 0)] * 3, 1 << 30, None)
        accepts = check_pass(n, clauses, hints[b])[0]                             # then the plain call reports no improvement, the cube one
        assert root[0] == 1 and root[1] == w[1] and np.array_equal(root[2], w[2]) and root[5] == w[4] + accepts
        half = rm.cube(n, clauses, hints[b], pens[b], [(0, 1)], 1 << 30, None)
        other = rm.cube(n, clauses, hints[b], pens[b], [(1, 1)], 1 << 30, None)
        assert min([r[1] for r in (half, other) if r[1] >= 0], default=-1) == w[1]


def test_start_models():
    inst, hints, pens = nc.small()
    pick = [b for b in range(len(inst)) if plain(True)[b][0] == 1 and plain(True)[b][1] > 0][:60]
    inst, hints, pens = [inst[b] for b in pick], [hints[b] for b in pick], [pens[b] for b in pick]
    best = [plain(True)[b] for b in pick]
    rng = np.random.RandomState(8)
    some = [nc.any_model(rm.inst_n(i), i[1]) for i in inst]
    wrong = []
    for (n, c), m in zip(inst, some):
        x = m.copy()
        while nc.satisfies(c, x):
            x = rng.randint(0, 2, size=len(m)).astype(np.float32)
        wrong.append(x)
    for budget, give in ((40, 1), (1 << 30, 0)):
        none = rm.run(inst, hints, pens, None, budget, give)
        # a model seeds cost and model, and the cost never rises above it (R4)
        seeded = rm.State(inst, hints, pens, some)
        far = [nm.distance(threshold(len(m), hints[b]), nm.penalty_list(len(m), pens[b]), m) for b, m in enumerate(some)]
        assert seeded.cost == far and all(np.array_equal(a, b) for a, b in zip(seeded.model, some))
        while seeded.cubes():
            checked_round(inst, seeded, budget, give)
            assert all(c <= f for c, f in zip(seeded.cost, far))
        assert seeded.status == none.status and seeded.cost == none.cost == [w[1] for w in best]
        assert sum(seeded.work) < sum(none.work)
        # an assignment that is not a model is ignored: the run is the one without a start
        ignored = rm.run(inst, hints, pens, wrong, budget, give)
        assert ignored.cost == none.cost and ignored.work == none.work and all(np.array_equal(a, b) for a, b in zip(ignored.model, none.model))
        # an optimal start: no cube ever improves -- with a budget above the tree every cube ends in round 1 -- and the model stays the
        # caller's
        optimal = rm.State(inst, hints, pens, [w[2] for w in best])
        while optimal.cubes():
            rec, first = checked_round(inst, optimal, budget, give)
            assert all(r[2] == -1 and r[5] == 0 for r in rec) and set(first) == {-1}
            assert budget < 1 << 30 or (optimal.cubes() == 0 and all(r[1] == 1 for r in rec))
        assert optimal.status == [1] * len(inst) and optimal.cost == [w[1] for w in best] and sum(optimal.improvements) == 0
        assert all(np.array_equal(a, w[2]) for a, w in zip(optimal.model, best))


def test_a_copied_state_finishes_the_same():
    inst, hints, pens = nc.small()
    more = cs.uniform_3sat(9, 20, (4.3,), 4)
    h2, p2 = nc.dress(more, 9)
    inst, hints, pens = inst[:150] + more, hints[:150] + h2, pens[:150] + p2
    state = rm.State(inst, hints, pens)
    for _ in range(3):
        rm.round(inst, state, 40, 1)
    assert state.cubes() > 0
    held = copy.deepcopy(state)
    while state.cubes():
        rm.round(inst, state, 40, 1)
    while held.cubes():
        rm.round(inst, held, 40, 1)
    for f in ('status', 'cost', 'work', 'improvements', 'rounds'):
        assert getattr(held, f) == getattr(state, f)
    assert all(np.array_equal(a, b) for a, b in zip(held.model, state.model))
    # other budgets and gives from the third round on: the same statuses and costs (R3), attained models
    again = rm.State(inst, hints, pens)
    for r in range(1 << 20):
        if not again.cubes():
            break
        rm.round(inst, again, 40 if r < 3 else 500, 1 if r < 3 else 3)
    assert again.status == state.status and again.cost == state.cost and all(attained(inst, again, b) for b in range(len(inst)))


def test_a_total_budget_leaves_an_upper_bound():
    inst = cs.uniform_3sat(5230, 30, (3.5, 4.0), 3)
    hints, pens = nc.dress(inst, 4200)
    full = rm.run(inst, hints, pens, None, 500, 2)
    total = sorted(full.work)[len(inst) // 2] // 2
    low = rm.run(inst, hints, pens, None, 500, 2, total=total)
    out = [b for b in range(len(inst)) if low.status[b] == -1]
    assert len(out) >= 2 and low.cubes() == 0
    for b in range(len(inst)):
        assert attained(inst, low, b)
        if b in out:
            assert low.work[b] >= total and (low.cost[b] < 0 or full.cost[b] < 0 or low.cost[b] >= full.cost[b])
        else:
            assert (low.status[b], low.cost[b]) == (full.status[b], full.cost[b])


def test_refusals_and_bad_penalties():
    n, clauses = 4, [[1, 2], [-1, 3], [2, -4]]
    for path in ([(1, 0)], [(0, 1), (1, 0)], [(0, 0)] * 5):
        with pytest.raises(ValueError):
            rm.cube(n, clauses, None, None, path, 10, None)
    wide = (1024, [[1, 2], [-1, 1024]])
    heavy = [np.array([1, 1, (1 << 20) + 1, 0]), None, np.array([0, 1 << 20, 1, 1]), np.array([0, -1, 1, 1])]
    batch = [(n, clauses), wide, (n, clauses), (n, clauses)]
    state = rm.State(batch, None, heavy)
    assert state.paths == [[], [], [[]], []] and state.status == [-3, -2, -1, -3]
    done = rm.run(batch, None, heavy, [np.ones(4), None, None, np.ones(4)], 5, 1)
    assert done.status == [-3, -2, 1, -3] and done.cost == [-1, -1, 1, -1] and done.work[0] == done.work[1] == done.work[3] == 0
    assert done.rounds == [0, 0, done.rounds[2], 0] and not done.model[0].any() and not done.model[3].any()
    assert rm.cube(n, clauses, None, None, [], 0, None)[0] == 1                   # budget <= 0: the default, far above this tree
    with pytest.raises(AssertionError):
        rm.cube(n, clauses, [0.5] * 3, None, [], 10, None)                        # one hint per variable
    with pytest.raises(AssertionError):
        rm.cube(n, clauses, None, heavy[0], [], 10, None)                         # a cube is never run on a penalty out of range


def test_header_and_symbols():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    m = re.search(r'#define PDP_EXACT_NEAREST_ROUND_BUDGET \(\(\(int64_t\)1\) << (\d+)\)', text)
    assert '#define PDP_ABI_VERSION 3' in text and m
    assert ("int pdp_exact_nearest_round(pdp_problem *p, const float *hint, const int32_t *penalty, const int64_t *cube_off, int64_t cubes, "
            "const int32_t *len, const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status, int64_t *cost, float *model, "
            "int64_t *work, int32_t *improvements, int32_t *first, int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, "
            "uint32_t *closed_out, int64_t *cube_cost, int64_t *cube_work, int64_t *cube_replay, int32_t *cube_improvements, "
            "void *stream);") in text
    from pdp import exact, native
    assert 'pdp_exact_nearest_round' in native.EXPORTED_SYMBOLS
    assert exact.NEAREST_ROUND_BUDGET == rm.ROUND_BUDGET == 1 << int(m.group(1))
    assert exact.MAX_PENALTY == native.EXACT_NEAREST_MAX_PENALTY == rm.MAX_PENALTY
    assert ['cube_off', 'len', 'bits', 'closed', 'hint', 'penalty', 'status', 'cost', 'model', 'work', 'improvements',
            'rounds'] == list(native.NearestState.FIELDS)
    assert hasattr(native.Problem, 'exact_nearest_begin') and hasattr(native.Problem, 'exact_nearest_round')
    assert hasattr(exact, 'nearest_rounds') and hasattr(exact, 'nearest_rounds_give') and exact.NEAREST_ROUNDS_WAVES_PER_SIMD >= 1
    with open(native.LIB_PATH, 'rb') as f:
        assert b'pdp_exact_nearest_round\0' in f.read()                           # the exported symbol, in the built library's string table


@pytest.mark.parametrize('kw', [dict(round_budget=0), dict(rounds=-1), dict(round_budget=1.5), dict(rounds=True)])
def test_nearest_model_rounds_refuses_bad_rounds(kw):
    from pdp import exact
    with pytest.raises(ValueError, match='round'):
        exact.nearest_model_rounds([exact.raw_item(2, [[1, 2]])], [np.zeros(2, dtype=np.float32)], **kw)


def test_nearest_model_itself_is_as_it_was():
    # the rounds are a call of their own: nearest_model keeps its signature and keeps refusing split='rounds'
    import inspect
    from pdp import exact
    assert list(inspect.signature(exact.nearest_model).parameters) == ['items', 'hints', 'penalties', 'budget', 'device', 'max_edges', 'split',
                                                                       'start', 'depths']
    with pytest.raises(ValueError, match='split must be'):
        exact.nearest_model([exact.raw_item(2, [[1, 2]])], [np.zeros(2, dtype=np.float32)], split='rounds')
    assert hasattr(exact, 'nearest_model_rounds')


def test_min_unsat_and_solution_mass_keep_refusing_rounds():
    from pdp import exact
    item = [exact.raw_item(2, [[1, 2]])]
    for call in (lambda: exact.min_unsat(item, split='rounds'),
                 lambda: exact.solution_mass(item, [np.full(2, 0.5, dtype=np.float32)], split='rounds')):
        with pytest.raises(ValueError, match='split must be'):
            call()


@pytest.mark.parametrize('argv,said', [(['--complete', '--complete-nearest-rounds', '3'], 'give --complete-nearest as well'),
                                       (['--complete', '--complete-nearest', '--complete-nearest-rounds', '3', '--complete-nearest-split', '2'],
                                        'without --complete-nearest-split'),
                                       (['--complete', '--complete-nearest', '--complete-nearest-rounds', '41'], 'from 0 to 40'),
                                       (['--complete', '--complete-nearest', '--complete-nearest-rounds', '-2'], 'from 0 to 40')])
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
    assert e.value.code == 2 and '--complete-nearest-rounds' in err and said in err
