"""The resumable nearest-model search on the GPU (pdp_exact_nearest_round with pdp_exact_count_expand, Problem.exact_nearest_begin /
exact_nearest_round, exact.nearest_model_rounds, satyr.py --complete --complete-nearest --complete-nearest-rounds): equal to its
Python statement (tests/exact_nearest_rounds_model.py) bit for bit, round by round, in status, cost, model, work, improvements, first,
every cube record, every checkpoint and every word of the expanded frontier; final status and cost equal to exact_nearest's and every
model checked on the host; the give = 0 identity; determinism over call, batch, grid and build; the HBM route and instances that are
too large; a thousand units of penalty 2^20 in one pass; a state continued on another handle; refusals with nothing written; the host entry points; the command
line."""
import ctypes
import faulthandler
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_nearest_cases as nc
import exact_nearest_model as nm
import exact_nearest_rounds_model as rm
from exact_min_unsat_model import threshold
from helpers import REPO

pytestmark = pytest.mark.gpu

PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
PAIRS = [(1, 0), (1, 3), (40, 1), (200, 8), (3000, 2)]  # reads per cube and round, levels given away; the last one runs several nodes a round
RECORDS = ('cube_off', 'cube_status', 'cube_cost', 'cube_work', 'cube_replay', 'cube_improvements', 'len_out', 'bits_out', 'closed_out', 'first')
RECORD_TYPES = [np.int64, np.int8, np.int64, np.int64, np.int64, np.int32, np.int32, np.int32, np.int32, np.int32]
UNIFORM_N, UNIFORM_RATIOS = (20, 30, 40), (3.5, 4.0, 4.5)
# the instances of wide_batch() do not end within any budget a test can pay for: they leave the frontier once their work has reached this
# total, by the driver's rule (exact.nearest_rounds_drop_spent, the model's drop_spent), and stay at status -1 with an upper bound
WIDE_TOTAL = 60_000
NO_TOTAL = 1 << 60
PLAIN_BUDGET = 3_000_000   # of the plain call the final answers are compared with: every instance but the wide ones ends far below it
STEP_LIMIT = 240        # seconds per test: a cube kernel that does not end is a hang, and ends the run with every thread's traceback


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def problem(inst):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment([exact.raw_item(n, c) for n, c in inst]), torch.device('cuda:0'))
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(inst))


@functools.lru_cache(maxsize=None)
def instances():
    """(instances, hints, mixed penalties, start models, total per instance): the host family (n <= 12), the two fans (the second prunes
    a flip before any pass), the fill case, uniform 3-SAT of n = 20 / 30 / 40 at ratios 3.5 / 4.0 / 4.5, and the wide batch (trails past
    128).  A start model per instance, in turn: a model where there is one, random bits, all false."""
    inst, hints, pens = [list(x) for x in nc.small()]
    for case in (nc.fan_case(60), nc.fan_case(150), nc.fill_case()):
        inst.append(case[0]); hints.append(case[1]); pens.append(case[2])
    for n in UNIFORM_N:
        u = cs.uniform_3sat(5200 + n, n, UNIFORM_RATIOS, 2)
        h, q = nc.dress(u, 4200)
        inst += u; hints += h; pens += q
    narrow = len(inst)
    w = nc.wide_batch()
    inst += w[0]; hints += w[1]; pens += w[2]
    inst = [(rm.inst_n(i), i[1]) for i in inst]
    rng = np.random.RandomState(12)
    start = []
    for b, (n, c) in enumerate(inst):
        m = nc.any_model(n, c) if b < narrow and b % 3 == 0 else None
        if m is None:
            m = rng.randint(0, 2, size=n).astype(np.float32) if b % 3 != 2 else np.zeros(n, dtype=np.float32)
        start.append(np.asarray(m, dtype=np.float32))
    total = np.array([NO_TOTAL] * narrow + [WIDE_TOTAL] * (len(inst) - narrow), dtype=np.int64)
    return tuple(inst), tuple(hints), tuple(pens), tuple(start), total


def flat(inst, per, dtype, fill):
    "one value per variable of the batch from one array (or None) per instance"
    return torch.from_numpy(np.concatenate([np.full(n, fill, dtype=dtype) if per is None or per[b] is None else np.asarray(per[b], dtype=dtype)
                                            for b, (n, _) in enumerate(inst)])).cuda()


def begin(p, inst, hints, pens, start):
    return p.exact_nearest_begin(flat(inst, hints, np.float32, 0.0), None if pens is None else flat(inst, pens, np.int32, 1),
                                 None if start is None else flat(inst, start, np.float32, 0.0))


def snapshot(state):
    "every tensor of a NearestState as numpy"
    return {f: getattr(state, f).cpu().numpy() for f in state.FIELDS}


def one_round(p, state, budget, give):
    "Problem.exact_nearest_round(stats=True): (open cubes, the records as a dict of numpy arrays)"
    made, rec = p.exact_nearest_round(state, budget, give, stats=True)
    rec = dict(zip(RECORDS, [t.cpu().numpy() for t in rec]))
    assert [rec[k].dtype for k in RECORDS] == RECORD_TYPES
    assert made == state.cubes == int(state.cube_off[-1].item())
    return made, rec


def model_snapshot(inst, mstate, W):
    off, ln, bits, closed = rm.frontier(mstate, W)
    hint = [np.zeros(n, dtype=np.float32) if mstate.hint(b) is None else np.asarray(mstate.hint(b), dtype=np.float32) for b, (n, _) in enumerate(inst)]
    pen = [np.ones(n, dtype=np.int32) if mstate.pen(b) is None else np.asarray(mstate.pen(b), dtype=np.int32) for b, (n, _) in enumerate(inst)]
    return dict(cube_off=off, len=ln, bits=bits, closed=closed, hint=np.concatenate(hint), penalty=np.concatenate(pen),
                status=np.array(mstate.status, dtype=np.int8), cost=np.array(mstate.cost, dtype=np.int64), model=np.concatenate(mstate.model),
                work=np.array(mstate.work, dtype=np.int64), improvements=np.array(mstate.improvements, dtype=np.int32),
                rounds=np.array(mstate.rounds, dtype=np.int32))


def model_round(inst, mstate, budget, give, W, whole=(), total=None, stats=None):
    "one round of the model in the layout of one_round's records, the State in snapshot's, and the State once more after the total budget"
    ran = rm.frontier(mstate, W)[0]
    rec, first = rm.round(inst, mstate, budget, give, whole, stats)
    ln, bits, closed = rm.pack([r[6] for r in rec], W)
    want = dict(cube_off=ran, cube_status=np.array([r[1] for r in rec], dtype=np.int8), cube_cost=np.array([r[2] for r in rec], dtype=np.int64),
                cube_work=np.array([r[3] for r in rec], dtype=np.int64), cube_replay=np.array([r[4] for r in rec], dtype=np.int64),
                cube_improvements=np.array([r[5] for r in rec], dtype=np.int32), len_out=ln, bits_out=bits, closed_out=closed,
                first=np.array(first, dtype=np.int32))
    after = model_snapshot(inst, mstate, W)
    if total is not None:
        rm.drop_spent(mstate, total)
    return want, after, model_snapshot(inst, mstate, W)


def words_of(inst):
    return rm.words(max([n for n, _ in inst if n <= rm.MAX_N] + [0]))


@functools.lru_cache(maxsize=None)
def model_trace(budget, give, mixed, started):
    """the model on the batch, run once per (pair, penalties, start): [(records, state after the round, state after the total budget)],
    the peak of open cubes per instance, the rounds every instance improved in, and the cubes that ended inside their replay"""
    inst, hints, pens, start, total = instances()
    inst = list(inst)
    W = words_of(inst)
    mstate = rm.State(inst, hints, pens if mixed else None, start if started else None)
    out, peak, improved, stats = [model_snapshot(inst, mstate, W)], np.zeros(len(inst), dtype=np.int64), np.zeros(len(inst), dtype=np.int64), {}
    while mstate.cubes():
        peak = np.maximum(peak, [len(p) for p in mstate.paths])
        out.append(model_round(inst, mstate, budget, give, W, total=total, stats=stats))
        improved += out[-1][0]['first'] >= 0
    return out, peak, improved, stats.get('in_replay', 0)


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


def in_lockstep(inst, p, state, trace, total=None):
    """the GPU against a model trace [(budget, give, records, state, state after the total budget)] round by round: every record, output
    and frontier word equal"""
    from pdp import exact
    same(snapshot(state), trace[0], 'begin')
    history = []
    for r, (budget, give, want, after, cut) in enumerate(trace[1:]):
        made, rec = one_round(p, state, budget, give)
        same(rec, want, 'records of round %d' % r)
        same(snapshot(state), after, 'state after round %d' % r)
        if total is not None:
            exact.nearest_rounds_drop_spent(state, total)
            same(snapshot(state), cut, 'state after the total budget of round %d' % r)
        history.append(rec)
    assert state.cubes == 0
    return state, history


def attained(inst, hints, pens, got):
    "per instance: cost -1 and a model of zeros, or a model of the instance at exactly that penalty distance from its hint"
    v0 = np.concatenate([[0], np.cumsum([n for n, _ in inst])])
    out = []
    for b, (n, cl) in enumerate(inst):
        m = got['model'][v0[b]:v0[b + 1]]
        if got['cost'][b] < 0:
            out.append(not m.any())
        else:
            out.append(nc.satisfies(cl, m) and nm.distance(threshold(n, hints[b]), nm.penalty_list(n, None if pens is None else pens[b]), m)
                       == got['cost'][b])
    return np.array(out)


@pytest.fixture(scope='module')
def batch():
    "the instances in one problem; exact_nearest of the same handle with the mixed penalties and with none, computed once"
    inst, hints, pens, start, total = instances()
    inst = list(inst)
    p = problem(inst)
    h = flat(inst, hints, np.float32, 0.0)
    plain = {m: [t.cpu().numpy() for t in p.exact_nearest(h, flat(inst, pens, np.int32, 1) if m else None, PLAIN_BUDGET, stats=True)]
             for m in (False, True)}
    return inst, p, plain


def test_the_inputs_meet_their_conditions():
    # conditions on the inputs, checked on the CPU model before anything runs on the GPU, so that the batch cannot go easy on the kernel
    inst = instances()[0]
    trace, peak, improved, _ = model_trace(40, 1, True, False)
    final = trace[-1][2]
    assert len(inst) >= 450 and 4 * int((final['status'] == 0).sum()) >= len(inst)        # a quarter is unsatisfiable
    assert ((final['rounds'] >= 10) & (peak >= 10)).any()                                 # long runs with many cubes open at once
    assert (improved >= 3).any()                                                          # a cost that falls in three different rounds
    assert model_trace(200, 8, True, False)[3] >= 20                                      # cubes ended in their replay by a sibling's bound
    assert (final['status'] == -1).sum() >= 8                                             # the total budget bites on the wide instances


@pytest.mark.parametrize('started', [False, True])
@pytest.mark.parametrize('mixed', [False, True])
@pytest.mark.parametrize('budget,give', PAIRS)
def test_equal_to_the_python_model_round_by_round(batch, budget, give, mixed, started):
    inst, p, plain = batch
    _, hints, pens, start, total = instances()
    pens = pens if mixed else None
    trace = model_trace(budget, give, mixed, started)[0]
    state = begin(p, inst, hints, pens, start if started else None)
    first = snapshot(state)
    state, history = in_lockstep(inst, p, state, [trace[0]] + [(budget, give) + t for t in trace[1:]], torch.from_numpy(total).cuda())
    got = snapshot(state)
    st, co, model, work, imp = plain[mixed]
    print('rounds budget %d give %d mixed %s start %s: %d rounds, frontier peak %d cubes, reads %.2f times the plain search'
          % (budget, give, mixed, started, len(history), max(len(h['cube_status']) for h in history),
             got['work'][st != -1].sum() / work[st != -1].sum()))
    ended = got['status'] != -1
    assert (ended[total == NO_TOTAL]).all() and (st[total == NO_TOTAL] != -1).all()        # every instance but the wide ones ends
    both = ended & (st != -1)
    assert np.array_equal(got['status'][both], st[both]) and np.array_equal(got['cost'][both], co[both]) and set(st[both].tolist()) == {0, 1}
    assert attained(inst, hints, pens, got).all()
    if started:
        seeded = first['cost'] >= 0
        assert seeded.sum() > 50 and (got['cost'][seeded] <= first['cost'][seeded]).all() and (got['cost'][seeded] >= 0).all()
    if give == 0 and not started:
        # one cube throughout: the plain search interrupted and resumed, wherever its check pass does not accept the hint (where it
        # does, the rounds follow the hint to the same model and count that leaf)
        accept = np.array([all(any((l > 0) == bool(threshold(n, hints[b])[abs(l) - 1]) for l in c if l != 0) for c in cl)
                           for b, (n, cl) in enumerate(inst)])
        assert accept.sum() > 20 and (both & ~accept).sum() > 250
        per = np.repeat(both, [n for n, _ in inst])
        assert np.array_equal(got['model'][per], model[per])
        assert np.array_equal(got['improvements'][both & ~accept], imp[both & ~accept])
        assert (got['improvements'][both & accept] == 1).all() and (imp[both & accept] == 0).all() and (got['cost'][both & accept] == 0).all()
        fresh = np.zeros(len(inst), dtype=np.int64)
        for h in history:
            np.add.at(fresh, np.repeat(np.arange(len(inst)), np.diff(h['cube_off'])), h['cube_work'] - h['cube_replay'])
        check = np.array([sum(next((j + 1 for j, l in enumerate(c) if (l > 0) == bool(threshold(n, hints[b])[abs(l) - 1])), len(c)) for c in
                              ([l for l in c if l != 0] for c in cl)) for b, (n, cl) in enumerate(inst)])
        assert np.array_equal((fresh + check)[both & ~accept], work[both & ~accept])
        assert all(len(h['cube_status']) <= len(inst) for h in history)
    # the work bound of a round: the replay, the budget, and one node (at most n + 1 passes of e reads and a branching pass of 2 e)
    node = np.array([(n + 3) * sum(len(c) for c in cl) for n, cl in inst], dtype=np.int64)
    for h in history:
        per = np.repeat(node, np.diff(h['cube_off']))
        stopped = h['cube_status'] < 0
        assert (h['cube_replay'] <= h['cube_work']).all() and (h['cube_work'] <= h['cube_replay'] + budget + per).all()
        assert (h['cube_work'][stopped] - h['cube_replay'][stopped] >= budget).all()
        assert (h['len_out'][~stopped] == 0).all() and set(h['cube_status'].tolist()) <= {-2, -1, 1}
        assert ((h['cube_cost'] >= 0) == (h['cube_improvements'] > 0)).all()
    assert got['rounds'].max() == len(history) >= 5


def test_deterministic_in_every_output_and_frontier_word(batch, monkeypatch):
    from pdp import exact, native
    inst, p, _ = batch
    _, hints, pens, start, total = instances()
    budget, give = 40, 2

    def rows(words):
        "the rows of a path array as integers, whatever the words per row: a lone instance has narrower rows than the batch"
        return tuple(sum(int(x) << (32 * k) for k, x in enumerate(r)) for r in words.view(np.uint32))

    def trace(prob, idx):
        "every record and every state of a run, per instance and round, in a comparable form"
        items = [inst[i] for i in idx]
        state = begin(prob, items, [hints[i] for i in idx], [pens[i] for i in idx], [start[i] for i in idx])
        cap = torch.from_numpy(total[list(idx)]).cuda()
        out = [[] for _ in items]
        v0 = np.concatenate([[0], np.cumsum([n for n, _ in items])])
        while state.cubes:
            _, rec = one_round(prob, state, budget, give)
            exact.nearest_rounds_drop_spent(state, cap)
            snap = snapshot(state)
            for j in range(len(items)):
                a, z = rec['cube_off'][j], rec['cube_off'][j + 1]
                b, y = snap['cube_off'][j], snap['cube_off'][j + 1]
                if z > a:
                    out[j].append(tuple(rec[k][a:z].tobytes() for k in RECORDS[1:7]) + (rows(rec['bits_out'][a:z]), rows(rec['closed_out'][a:z]),
                                  int(rec['first'][j]), snap['len'][b:y].tobytes(), rows(snap['bits'][b:y]), rows(snap['closed'][b:y]),
                                  snap['model'][v0[j]:v0[j + 1]].tobytes(), int(snap['cost'][j]), int(snap['work'][j]),
                                  int(snap['improvements'][j]), int(snap['status'][j]), int(snap['rounds'][j])))
        return out

    everything = list(range(len(inst)))
    a = trace(p, everything)
    assert sum(len(r) for r in a) > len(inst) + 100 and max(len(r) for r in a) >= 5      # many instances run several rounds
    assert a == trace(p, everything)                                                      # a second run on one handle
    order = [int(i) for i in np.random.RandomState(6).permutation(len(inst))]
    assert [a[i] for i in order] == trace(problem([inst[i] for i in order]), order)       # a shuffled batch
    for i in list(range(0, len(inst), 97)) + [len(inst) - 3, len(inst) - 1]:             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            assert [a[i]] == trace(problem([inst[i]]), [i])
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every cube, one after the other
    one = trace(p, everything)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    assert a == one
    state = p.exact_nearest_begin()
    p.exact_nearest_round(state, budget, give)
    assert p.exact_last_grid() > 1
    prev = native.use_build('fast')
    try:
        fast = trace(problem(inst), everything)
    finally:
        native.use_build(prev)
    assert a == fast


def run_model(inst, hints, pens, start, budget, give, W, whole=()):
    mstate = rm.State(inst, hints, pens, start)
    trace = [model_snapshot(inst, mstate, W)]
    while mstate.cubes():
        trace.append((budget, give) + model_round(inst, mstate, budget, give, W, whole))
    return trace


def test_hbm_route_keeps_one_cube():
    big, bh, bp = nc.slab_case()
    few, fh, fp = [list(x[:40]) for x in nc.small()]
    inst = [(rm.inst_n(i), i[1]) for i in few[:20] + [big] + few[20:]]
    hints, pens = fh[:20] + [bh] + fh[20:], fp[:20] + [bp] + fp[20:]
    W = words_of(inst)
    # one node a round: the small instances are cut up, the large one keeps its one cube
    trace = run_model(inst, hints, pens, None, 1, 4, W, whole={20})
    p = problem(inst)
    state, history = in_lockstep(inst, p, begin(p, inst, hints, pens, None), trace)
    mine = [h for h in history if h['cube_off'][21] > h['cube_off'][20]]
    assert len(mine) >= 3 and all(h['cube_off'][21] - h['cube_off'][20] == 1 for h in mine)          # several rounds, never expanded
    assert any(h['cube_off'][20] > 20 for h in history)                                   # while the instances before it were
    got = snapshot(state)
    want = nc.slab_result()
    assert (got['status'][20], got['cost'][20], got['improvements'][20]) == (want[0], want[1], want[4]) and got['rounds'][20] == len(mine)
    v0 = sum(n for n, _ in inst[:20])
    assert np.array_equal(got['model'][v0:v0 + inst[20][0]], want[2])                     # one cube: the plain search's model
    # two cubes on the HBM route are refused: its working arrays are per instance
    from pdp import native
    bad = begin(p, inst, hints, pens, None)
    bad.cube_off[21:] += 1
    for f in ('len', 'bits', 'closed'):
        t = getattr(bad, f)
        setattr(bad, f, torch.cat([t[:21], t[20:21], t[21:]]).contiguous())
    with pytest.raises(native.NativeError, match='instance 20 is on the HBM route'):
        p.exact_nearest_round(bad, 1, 0)


def test_too_many_variables_and_a_thousand_heavy_units():
    from pdp import exact, native
    few, fh, fp = [list(x[:6]) for x in nc.small()]
    few = [(rm.inst_n(i), i[1]) for i in few]
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    edge = (1023, [[1, 2], [-1, 1023]])
    units = (1000, [[i + 1] for i in range(1000)])                                        # one pass of 16 chunks, cost 1000 * 2^20
    inst = few[:3] + [wide] + few[3:] + [edge, units]
    rng = np.random.RandomState(2)
    hints = fh[:3] + [rng.randint(0, 2, size=1024).astype(np.float32)] + fh[3:] + [np.ones(1023, dtype=np.float32), np.zeros(1000, dtype=np.float32)]
    pens = fp[:3] + [np.ones(1024, dtype=np.int32)] + fp[3:] + [np.full(1023, 3, dtype=np.int32), np.full(1000, nc.CAP, dtype=np.int32)]
    W = words_of(inst)
    trace = run_model(inst, hints, pens, None, 30, 2, W)
    p = problem(inst)
    state, history = in_lockstep(inst, p, begin(p, inst, hints, pens, None), trace)
    got = snapshot(state)
    assert got['status'][3] == -2 and got['status'][7] == 1 and got['bits'].shape == (0, 32)
    assert (got['cost'][3], got['work'][3], got['rounds'][3]) == (-1, 0, 0) and not got['model'][sum(n for n, _ in inst[:3]):][:1024].any()
    assert got['cost'][8] == 1000 << 20 and got['status'][8] == 1 and got['model'][-1000:].all() and got['improvements'][8] == 1
    assert all(h['first'][3] == -1 for h in history)
    assert history[0]['cube_off'].tolist() == [0, 1, 2, 3, 3, 4, 5, 6, 7, 8]              # no cube on the wide instance
    bad = begin(p, inst, hints, pens, None)
    bad.cube_off[4:] += 1
    for f in ('len', 'bits', 'closed'):
        t = getattr(bad, f)
        setattr(bad, f, torch.cat([t[:1], t]).contiguous())
    with pytest.raises(native.NativeError, match='cube 3 is on an instance of more than 1023 variables'):
        p.exact_nearest_round(bad, 1, 0)
    # the driver sends the wide instance to the plain call
    raw = [exact.raw_item(n, c) for n, c in inst]
    st, co, models, work, used = exact.nearest_model_rounds(raw, hints, pens, round_budget=30, depths=True)
    base = exact.nearest_model(raw, hints, pens)
    assert np.array_equal(st, base[0]) and np.array_equal(co, base[1]) and st[3] == 1 and work[3] == base[3][3] > 0 and used[3] == 0
    assert np.array_equal(models[3], base[2][3]) and used.dtype == np.int32 and (np.delete(used, 3) >= 1).all()


def test_a_state_continues_on_another_problem(batch):
    from pdp import exact
    inst, p, plain = batch
    _, hints, pens, start, total = instances()
    cap = torch.from_numpy(total).cuda()
    state = begin(p, inst, hints, pens, None)
    for _ in range(3):
        assert p.exact_nearest_round(state, 200, 2) > 0
    held = state.cpu()
    assert all(getattr(held, f).device.type == 'cpu' for f in held.FIELDS) and held.cubes == state.cubes
    before = snapshot(state)
    q = problem(inst)                                                                     # a new handle of the same items
    moved = held.to(q.device)
    rounds = 0
    while moved.cubes:
        q.exact_nearest_round(moved, 5000, 1)
        p.exact_nearest_round(state, 5000, 1)
        exact.nearest_rounds_drop_spent(moved, cap)
        exact.nearest_rounds_drop_spent(state, cap)
        rounds += 1
    same(snapshot(moved), snapshot(state), 'continued')
    same(snapshot(held), before, 'the copy is left alone')
    got = snapshot(moved)
    both = (got['status'] != -1) & (plain[True][0] != -1)
    assert both.sum() > 430 and np.array_equal(got['status'][both], plain[True][0][both]) and np.array_equal(got['cost'][both], plain[True][1][both])
    assert attained(inst, hints, pens, got).all() and rounds >= 2


def test_caller_made_frontier_of_closed_paths(batch):
    # all 2^d closed paths of depth d on one instance are pdp_exact_nearest_split's cubes: between them they hold the instance's minimum
    # (where the tree is shallower than the path, as in the small instance here, a leaf is met inside the path)
    inst, p, plain = batch
    _, hints, pens, _, _ = instances()
    st, co = plain[True][0], plain[True][1]
    v0 = np.concatenate([[0], np.cumsum([n for n, _ in inst])])
    small = next(j for j, (n, _) in enumerate(inst) if 5 <= n <= 8 and st[j] == 1 and co[j] > 0)
    unsat = next(j for j in range(len(inst) - 1, 0, -1) if st[j] == 0 and inst[j][0] >= 20)
    hard = next(j for j in range(len(inst) - 1, 0, -1) if st[j] == 1 and co[j] > 0 and inst[j][0] == 40)
    d = 5
    for j in (small, unsat, hard):
        for f_budget in (0, 300):
            state = begin(p, inst, hints, pens, None)
            ln, bits, closed = rm.pack([[((i >> (d - 1 - k)) & 1, 1) for k in range(d)] for i in range(1 << d)], state.bits.size(1))
            off = np.zeros(len(inst) + 1, dtype=np.int64)
            off[j + 1:] = 1 << d
            state.cube_off, state.len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
            state.bits, state.closed = torch.from_numpy(bits).cuda(), torch.from_numpy(closed).cuda()
            while state.cubes:
                p.exact_nearest_round(state, f_budget, 1)
            got = snapshot(state)
            assert (got['status'][j], got['cost'][j]) == (st[j], co[j]) and (got['status'][np.arange(len(inst)) != j] < 0).all()
            assert attained(inst, hints, pens, got)[j] and not np.delete(got['model'], np.arange(v0[j], v0[j + 1])).any()
            assert (np.delete(got['cost'], j) == -1).all()


def test_refusals_write_nothing(batch):
    from pdp import native
    from pdp.factorgraph import dataset
    inst, p, _ = batch
    _, hints, pens, start, _ = instances()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    r2 = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        r2.exact_nearest_begin()
    L = native.lib()
    one = torch.zeros(8, dtype=torch.int64, device=p.device)
    assert L.pdp_exact_nearest_round(r2._h, None, None, native.ptr(one), ctypes.c_int64(0), None, None, None, ctypes.c_int64(1), native.ptr(one),
                                     native.ptr(one), native.ptr(one), native.ptr(one), native.ptr(one), native.ptr(one), None, None, None, None,
                                     None, None, None, None, None) == 4
    good = begin(p, inst, hints, pens, start)
    p.exact_nearest_round(good, 1, 2)
    p.exact_nearest_round(good, 1, 2)
    assert good.cubes > 50
    base = snapshot(good)

    def broken(field, at, value):
        s = good.to(p.device)
        getattr(s, field).view(-1)[at] = value
        return s

    W = good.bits.size(1)
    c = int(np.nonzero(base['len'] >= 2)[0][-1])
    owner = int(np.searchsorted(base['cube_off'], c, side='right')) - 1
    v0 = np.concatenate([[0], np.cumsum([n for n, _ in inst])])
    pair = broken('closed', c * W, int(base['closed'][c, 0]) & ~3 | 1)                    # level 2 of cube c: not closed,
    pair.bits.view(-1)[c * W] = int(base['bits'][c, 0]) | 2                               # and on its other polarity: the pair (1, 0)
    idle = int(np.nonzero(np.diff(base['cube_off']) == 0)[0][0])                           # an instance without a cube: its penalties are not read
    cases = [(broken('cube_off', 0, 1), 'cube_off must start at 0.*instance 0'),
             (broken('cube_off', 7, int(base['cube_off'][8]) + 1), 'cube_off must start at 0, never fall.*instance 7'),
             (broken('cube_off', len(inst), int(base['cube_off'][-1]) - 1), r'cube_off must start at 0.*instance %d' % (len(inst) - 1)),
             (broken('len', c, -1), 'length of cube %d is not in 0' % c),
             (broken('len', c, 1 << 20), 'length of cube %d is not in 0' % c),
             (broken('len', c, inst[owner][0] + 1), 'length of cube %d is not in 0' % c),
             (pair, r'cube %d has a level on its other polarity that is not closed' % c),
             (broken('penalty', int(v0[owner + 1]) - 1, (1 << 20) + 1), r'instance %d has a cube and a penalty outside 0 .. 2\^20' % owner),
             (broken('penalty', int(v0[owner]), -1), r'instance %d has a cube and a penalty outside 0 .. 2\^20' % owner)]
    for s, said in cases:
        before = snapshot(s)
        with pytest.raises(native.NativeError, match=said) as e:
            p.exact_nearest_round(s, 1, 1)
        assert 'pdp_exact_nearest_round: ' in str(e.value)
        same(snapshot(s), before, said)                                                   # answers and frontier as they were
    lazy = broken('penalty', int(v0[idle]), -5)
    assert p.exact_nearest_round(lazy, 1, 1) > 0                                          # no cube, no complaint
    # begin: an instance with a penalty out of range gets status -3 and no cube, and no start model
    q = flat(inst, pens, np.int32, 1)
    q[int(v0[5])] = (1 << 20) + 1
    q[int(v0[9 + 1]) - 1] = -1
    marked = p.exact_nearest_begin(flat(inst, hints, np.float32, 0.0), q, flat(inst, start, np.float32, 0.0))
    ms = snapshot(marked)
    assert ms['status'][[5, 9]].tolist() == [-3, -3] and (np.diff(ms['cube_off'])[[5, 9]] == 0).all() and (ms['cost'][[5, 9]] == -1).all()
    assert marked.cubes == len(inst) - 2 and (np.delete(ms['status'], [5, 9]) == -1).all()
    while marked.cubes and marked.rounds.max() < 3:
        p.exact_nearest_round(marked, 3000, 1)
    ms = snapshot(marked)
    assert ms['status'][[5, 9]].tolist() == [-3, -3] and (ms['work'][[5, 9]] == 0).all() and (ms['rounds'][[5, 9]] == 0).all()
    # the Python layer: the state's tensors, the hints, the budget and give
    for field, wrong in (('len', good.len.to(torch.int64)), ('bits', good.bits[:, :0]), ('model', good.model.cpu()), ('work', good.work[:-1]),
                         ('hint', good.hint.to(torch.float64)), ('status', good.status.to(torch.int32)), ('cost', good.cost.to(torch.int32)),
                         ('penalty', good.penalty.to(torch.int64)), ('improvements', good.improvements[:-1])):
        s = good.to(p.device)
        setattr(s, field, wrong)
        with pytest.raises(native.NativeError, match='state.%s must be' % field):
            p.exact_nearest_round(s)
    for kw in (dict(budget=1.5), dict(budget=True), dict(give=-1), dict(give='2'), dict(give=1024)):
        with pytest.raises(ValueError):
            p.exact_nearest_round(good, **kw)
    with pytest.raises(ValueError):
        p.exact_nearest_round(p.exact_solve_begin())
    for name, wrong in (('hints', good.hint[:-1]), ('hints', good.hint.cpu()), ('hints', good.hint.to(torch.float64)), ('hints', [0.5] * p.V),
                        ('penalties', good.penalty.to(torch.int64)), ('start', good.model[:-1])):
        with pytest.raises(ValueError, match='%s must be' % name):
            p.exact_nearest_begin(**{name: wrong})
    outs = [torch.full((good.cubes,), -7, dtype=torch.int8, device=p.device), torch.full((good.cubes,), -7, dtype=torch.int32, device=p.device),
            torch.full((good.cubes, W), -7, dtype=torch.int32, device=p.device), torch.full((good.cubes, W), -7, dtype=torch.int32, device=p.device)]
    first = torch.full((p.B,), -7, dtype=torch.int32, device=p.device)
    too_many = L.pdp_exact_nearest_round(p._h, native.ptr(good.hint), native.ptr(good.penalty), native.ptr(good.cube_off),
                                         ctypes.c_int64((1 << 22) + 1), native.ptr(good.len), native.ptr(good.bits), native.ptr(good.closed),
                                         ctypes.c_int64(1), native.ptr(good.status), native.ptr(good.cost), native.ptr(good.model),
                                         native.ptr(good.work), native.ptr(good.improvements), native.ptr(first), *[native.ptr(t) for t in outs],
                                         None, None, None, None, None)
    assert too_many != native.PDP_OK and b'a frontier holds 0 .. 2^22' in L.pdp_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs + [first])
    same(snapshot(good), base, 'the good state')


def test_nearest_model_rounds_on_segments_and_items_without_a_literal():
    from pdp import exact
    few, fh, fp = [list(x[:100]) for x in nc.small()]
    uni = cs.uniform_3sat(5230, 30, UNIFORM_RATIOS, 3)
    uh, up = nc.dress(uni, 4200)
    inst = few + uni
    hints = [np.array([1, 0, np.nan], dtype=np.float32), None] + fh + uh + [np.array([0.2, 0.9, 1, 0], dtype=np.float32)]
    pens = [None, None] + fp + up + [None]
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + [exact.raw_item(4, [[]])]
    base = exact.nearest_model(raw, hints, pens)
    assert set(base[0].tolist()) == {0, 1} and base[0][0] == 1 and base[0][1] == 0 and base[0][-1] == 0

    def valid(got, proved):
        for (n, c), h, q, m, co, st in zip(inst, hints[2:-1], pens[2:-1], got[2][2:-1], got[1][2:-1], got[0][2:-1]):
            assert m.dtype == np.float32 and len(m) == n
            assert (co == -1 and not m.any()) or (nc.satisfies(c, m) and nm.distance(threshold(n, h), nm.penalty_list(n, q), m) == co)
            assert not proved or st in (0, 1)

    for max_edges in (exact.MAX_EDGES, 400):
        got = exact.nearest_model_rounds(raw, hints, pens, round_budget=2000, max_edges=max_edges, depths=True)
        assert len(got) == 5 and np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        assert (got[0].dtype, got[1].dtype, got[3].dtype, got[4].dtype) == (np.int8, np.int64, np.int64, np.int32)
        valid(got, True)
        assert [m.tolist() for m in (got[2][0], got[2][1], got[2][-1])] == [[1, 0, 0], [0, 0], [0, 0, 0, 0]]
        assert got[3][0] == got[3][1] == got[3][-1] == 0 and (got[4][2:-1] >= 1).all()
        assert (got[4][-10:-1] > 1).sum() >= 3
    assert len(exact.nearest_model_rounds(raw[:5], hints[:5], pens[:5])) == 4
    # start models: a model seeds, an assignment that is none is ignored
    start = [None, None] + [nc.any_model(n, c) if b % 2 == 0 else None for b, (n, c) in enumerate(inst)] + [None]
    seeded = exact.nearest_model_rounds(raw, hints, pens, round_budget=2000, start=start)
    assert np.array_equal(seeded[0], base[0]) and np.array_equal(seeded[1], base[1])
    valid(seeded, True)
    # a total budget: the rows that reach it end unproved with a valid upper bound, the others as before
    total = int(np.median(base[3][-10:-1]))
    low = exact.nearest_model_rounds(raw, hints, pens, budget=total, round_budget=500)
    out = low[0] == -1
    assert out.sum() >= 2 and np.array_equal(low[0][~out], base[0][~out]) and np.array_equal(low[1][~out], base[1][~out])
    assert (low[3][out] >= total).all() and ((low[1][out] == -1) | (base[1][out] == -1) | (low[1][out] >= base[1][out])).all()
    valid(low, False)
    few_rounds = exact.nearest_model_rounds(raw, hints, pens, round_budget=100, rounds=2)
    assert (few_rounds[0] == -1).sum() >= 5 and np.array_equal(few_rounds[0][few_rounds[0] != -1], base[0][few_rounds[0] != -1])
    valid(few_rounds, False)
    # a penalty out of range: status -3, cost 0 and a model of zeros, as in the plain call
    heavy = list(pens)
    heavy[4] = np.full(int(raw[4][0]), (1 << 20) + 1, dtype=np.int64)
    a, b = exact.nearest_model_rounds(raw[:8], hints[:8], heavy[:8]), exact.nearest_model(raw[:8], hints[:8], heavy[:8])
    assert a[0][4] == b[0][4] == -3 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not a[2][4].any() and a[3][4] == 0


def test_most_probable_models_through_map_penalties():
    # exact.map_penalties turns a soft prediction into (hint, penalties); the nearest model in rounds is the most probable one, by brute force
    from pdp import exact
    inst = [i for i in cs.family() if 4 <= rm.inst_n(i) <= 10][:60]
    rng = np.random.RandomState(14)
    soft = [np.round(rng.rand(rm.inst_n(i)), 2) for i in inst]
    dressed = [exact.map_penalties(w) for w in soft]
    hints, pens = [d[0] for d in dressed], [d[1] for d in dressed]
    got = exact.nearest_model_rounds([exact.raw_item(rm.inst_n(i), i[1]) for i in inst], hints, pens, round_budget=60)
    sat = 0
    for (n, c), h, q, st, co, m in zip(inst, hints, pens, got[0], got[1], got[2]):
        n = rm.inst_n((n, c))
        least = nc.brute(n, c, threshold(n, h), nm.penalty_list(n, q))[0]
        assert (st, co) == ((1, least) if least is not None else (0, -1))
        assert least is None or (nc.satisfies(c, m) and nm.distance(threshold(n, h), nm.penalty_list(n, q), m) == least)
        sat += least is not None
    assert sat >= 20


def test_cli_complete_nearest_rounds(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    from exact_min_unsat_cases import threshold_3sat
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(31)
    for i in range(40):
        n, clauses = threshold_3sat(rng, 30, 126)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete', '--complete-nearest']
    own, _ = _run(argv[:-2], 1, str(tmp_path / 'own.jsonl'), 0)                           # PDP's own assignments: the hints
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-nearest-rounds', '9'], 1, str(tmp_path / 'deep.jsonl'), 0)
    assert len(base) == len(deep) == 40
    searched = several = 0
    moved = ('nearest_solution', 'nearest_work', 'nearest_rounds')
    for o, b, d in zip(own, base, deep):
        r, rb, o = json.loads(d), json.loads(b), json.loads(o)
        assert 'nearest_rounds' not in rb
        if rb['complete'] != 1:
            assert d == b                                                                 # byte-identical to the run without the flag
            continue
        assert list(r)[-2:] == ['nearest_work', 'nearest_rounds'] and list(r)[:-1] == list(rb)
        assert {k: v for k, v in r.items() if k not in moved} == {k: v for k, v in rb.items() if k not in moved}
        assert rb['nearest_proved'] == 1 and r['nearest_proved'] == 1 and r['nearest'] == rb['nearest'] and r['nearest_work'] > 0
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        assert len(r['nearest_solution']) == n and nc.satisfies(clauses, r['nearest_solution'])
        assert r['nearest'] == sum(x != y for x, y in zip(r['nearest_solution'], o['solution']))
        searched += 1
        several += r['nearest_rounds'] > 1
    assert searched >= 10 and several >= 3
