"""The resumable deciding search on the GPU (pdp_exact_solve_round with pdp_exact_count_expand, Problem.exact_solve_begin /
exact_solve_round, exact.solve_items(split='rounds'), satyr.py --complete --complete-rounds): equal to its Python statement
(tests/exact_solve_rounds_model.py) bit for bit, round by round, in status, model, work, first, every cube record, every checkpoint and
every word of the expanded frontier; final status equal to exact_solve's and every model checked on the host; the give = 0 identity;
determinism over call, batch, grid and build; the HBM route and instances that are too large; a state continued on another handle;
refusals with nothing written; the host entry points; the command line."""
import ctypes
import faulthandler
import functools
import json
import os

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_model as em
import exact_solve_rounds_model as sm
from helpers import REPO

pytestmark = pytest.mark.gpu

PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
PAIRS = [(1, 0), (1, 3), (40, 1), (200, 8), (3000, 2)]  # reads per cube and round, levels given away; the last one runs several nodes a round
RECORDS = ('cube_off', 'cube_status', 'cube_work', 'cube_replay', 'len_out', 'bits_out', 'closed_out', 'first')
UNIFORM = ((20, 20), (30, 30), (40, 40))               # (seed, n) of the uniform 3-SAT part, two instances at each of the ratios
RATIOS = (4.0, 4.3, 5.0)
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


def widen(inst):
    return [(sm.inst_n(i), i[1]) for i in inst]


@functools.lru_cache(maxsize=None)
def instances():
    "about 440 instances: the host family (n <= 12), the two fans, uniform 3-SAT of n = 20 / 30 / 40 at ratios 4.0 / 4.3 / 5.0"
    uniform = [i for seed, n in UNIFORM for i in cs.uniform_3sat(seed, n, RATIOS, 2)]
    return tuple(widen(cs.family() + [cs.fan(k) for k in cs.FAN_K] + uniform)), len(uniform)


@functools.lru_cache(maxsize=None)
def hints_for(hinted):
    """None, or one array per instance: every third instance has a value for every variable (so exact_solve's check pass runs), the others
    hold NaNs"""
    if not hinted:
        return None
    rng = np.random.RandomState(11)
    out = []
    for j, (n, _) in enumerate(instances()[0]):
        h = rng.rand(n).astype(np.float32)
        if j % 3:
            h[rng.rand(n) < 0.35] = np.nan
        out.append(h)
    return tuple(out)


def flat_hints(inst, hints):
    return None if hints is None else torch.from_numpy(np.concatenate(hints)).cuda()


def snapshot(state):
    "every tensor of a SolveState as numpy"
    return {f: getattr(state, f).cpu().numpy() for f in state.FIELDS}


def one_round(p, state, budget, give):
    "Problem.exact_solve_round(stats=True): (open cubes, the records as a dict of numpy arrays)"
    made, rec = p.exact_solve_round(state, budget, give, stats=True)
    rec = dict(zip(RECORDS, [t.cpu().numpy() for t in rec]))
    assert [rec[k].dtype for k in RECORDS] == [np.int64, np.int8, np.int64, np.int64, np.int32, np.int32, np.int32, np.int32]
    assert made == state.cubes == int(state.cube_off[-1].item())
    return made, rec


def model_snapshot(inst, mstate, W):
    off, ln, bits, closed = sm.frontier(mstate, W)
    hint = [np.full(n, np.nan, dtype=np.float32) if mstate.hint(b) is None else np.asarray(mstate.hint(b), dtype=np.float32)
            for b, (n, _) in enumerate(inst)]
    return dict(cube_off=off, len=ln, bits=bits, closed=closed, hint=np.concatenate(hint), status=np.array(mstate.status, dtype=np.int8),
                model=np.concatenate(mstate.model), work=np.array(mstate.work, dtype=np.int64), rounds=np.array(mstate.rounds, dtype=np.int32))


def model_round(inst, mstate, budget, give, W, whole=()):
    "one round of the model in the layout of one_round's records, and the State in snapshot's"
    ran = sm.frontier(mstate, W)[0]
    rec, first = sm.round(inst, mstate, budget, give, whole)
    ln, bits, closed = sm.pack([r[4] for r in rec], W)
    want = dict(cube_off=ran, cube_status=np.array([r[1] for r in rec], dtype=np.int8), cube_work=np.array([r[2] for r in rec], dtype=np.int64),
                cube_replay=np.array([r[3] for r in rec], dtype=np.int64), len_out=ln, bits_out=bits, closed_out=closed,
                first=np.array(first, dtype=np.int32))
    return want, model_snapshot(inst, mstate, W)


def words_of(inst):
    return sm.words(max([n for n, _ in inst if n <= sm.MAX_N] + [0]))


@functools.lru_cache(maxsize=None)
def model_trace(budget, give, hinted):
    "the model on the batch, run once per (pair, hints): [(records, state after the round)] and the peak of open cubes per instance"
    inst = list(instances()[0])
    W = words_of(inst)
    mstate = sm.State(inst, hints_for(hinted))
    out, peak = [model_snapshot(inst, mstate, W)], np.zeros(len(inst), dtype=np.int64)
    while mstate.cubes():
        peak = np.maximum(peak, [len(p) for p in mstate.paths])
        out.append(model_round(inst, mstate, budget, give, W))
    return out, peak


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


def in_lockstep(inst, p, hints, trace):
    "the GPU against a model trace [(budget, give, records, state)] round by round: every record, output and frontier word equal"
    state = p.exact_solve_begin(flat_hints(inst, hints))
    same(snapshot(state), trace[0], 'begin')
    history = []
    for r, (budget, give, want, after) in enumerate(trace[1:]):
        made, rec = one_round(p, state, budget, give)
        same(rec, want, 'records of round %d' % r)
        same(snapshot(state), after, 'state after round %d' % r)
        history.append(rec)
    assert state.cubes == 0
    return state, history


def satisfied(inst, model):
    "per instance: does its slice of ``model`` satisfy every clause"
    v0 = np.concatenate([[0], np.cumsum([n for n, _ in inst])])
    return np.array([all(any((model[v0[b] + abs(l) - 1] > 0.5) == (l > 0) for l in c) for c in cl) for b, (_, cl) in enumerate(inst)])


@pytest.fixture(scope='module')
def batch():
    "the instances in one problem; exact_solve of the same handle without and with the hints, computed once"
    inst = list(instances()[0])
    p = problem(inst)
    plain = {h: [t.cpu().numpy() for t in p.exact_solve(hints=flat_hints(inst, hints_for(h)))] for h in (False, True)}
    return inst, p, plain


def test_the_inputs_meet_their_conditions():
    # conditions on the inputs, checked on the CPU model before anything runs on the GPU
    inst, uniform = instances()
    status = [em.search(n, c)[0] for n, c in inst[-uniform:]]
    assert uniform == 18 and 3 * sum(s == 0 for s in status) >= uniform
    trace, peak = model_trace(40, 1, False)
    rounds = trace[-1][1]['rounds']
    assert ((rounds >= 10) & (peak >= 8)).any()
    assert len(inst) >= 430


@pytest.mark.parametrize('hinted', [False, True])
@pytest.mark.parametrize('budget,give', PAIRS)
def test_equal_to_the_python_model_round_by_round(batch, budget, give, hinted):
    inst, p, plain = batch
    trace, _ = model_trace(budget, give, hinted)
    state, history = in_lockstep(inst, p, hints_for(hinted), [trace[0]] + [(budget, give) + t for t in trace[1:]])
    got = snapshot(state)
    st, model, work = plain[hinted]
    print('rounds budget %d give %d hints %s: %d rounds, frontier peak %d cubes, reads %.2f times the plain search'
          % (budget, give, hinted, len(history), max(len(h['cube_status']) for h in history), got['work'].sum() / work.sum()))
    assert np.array_equal(got['status'], st) and set(st.tolist()) == {0, 1}
    assert satisfied(inst, got['model'])[st == 1].all() and not got['model'][np.repeat(st, [n for n, _ in inst]) == 0].any()
    few = len(cs.family())
    assert [s == 1 for s in st[:few]] == [b[0] > 0 for b in cs.family_brute()] and st[few:few + 2].tolist() == [1, 1]
    if give == 0:
        # one cube throughout: the plain search interrupted and resumed, wherever its check pass does not accept the hints
        hints = hints_for(hinted)
        accept = np.array([hinted and not np.isnan(hints[b]).any() and em.check_reads(c, (hints[b] > 0.5).astype(np.float32))[1]
                           for b, (n, c) in enumerate(inst)])
        assert hinted == bool(accept.any()) and (~accept).sum() > 300
        per = np.repeat(accept, [n for n, _ in inst])
        assert np.array_equal(got['model'][~per], model[~per])
        fresh = np.zeros(len(inst), dtype=np.int64)
        for h in history:
            np.add.at(fresh, np.repeat(np.arange(len(inst)), np.diff(h['cube_off'])), h['cube_work'] - h['cube_replay'])
        check = np.array([em.check_reads(c, (hints[b] > 0.5).astype(np.float32))[0] if hinted and not np.isnan(hints[b]).any() else 0
                          for b, (n, c) in enumerate(inst)])
        assert np.array_equal((fresh + check)[~accept], work[~accept])
        assert all(len(h['cube_status']) <= len(inst) for h in history)
    # the work bound of a round: the replay, the budget, and one node (at most n + 1 passes of e reads and a branching pass of 2 e)
    node = np.array([(n + 3) * sum(len(c) for c in cl) for n, cl in inst], dtype=np.int64)
    dropped = 0
    for h in history:
        per = np.repeat(node, np.diff(h['cube_off']))
        stopped = h['cube_status'] < 0
        assert (h['cube_replay'] <= h['cube_work']).all() and (h['cube_work'] <= h['cube_replay'] + budget + per).all()
        assert (h['cube_work'][stopped] - h['cube_replay'][stopped] >= budget).all()
        assert (h['len_out'][~stopped] == 0).all() and set(h['cube_status'].tolist()) <= {-2, -1, 0, 1}
        dropped += int((h['cube_status'] == -2).sum())
    assert (dropped > 0) == (give > 0)
    assert got['rounds'].max() == len(history) >= 5


def test_deterministic_in_every_output_and_frontier_word(batch, monkeypatch):
    from pdp import native
    inst, p, _ = batch
    budget, give = 40, 2
    hints = hints_for(True)

    def rows(words):
        "the rows of a path array as integers, whatever the words per row: a lone instance has narrower rows than the batch"
        return tuple(sum(int(x) << (32 * k) for k, x in enumerate(r)) for r in words.view(np.uint32))

    def trace(prob, items, hint):
        "every record and every state of a run, per instance and round, in a comparable form"
        state, out = prob.exact_solve_begin(flat_hints(items, hint)), [[] for _ in items]
        v0 = np.concatenate([[0], np.cumsum([n for n, _ in items])])
        while state.cubes:
            _, rec = one_round(prob, state, budget, give)
            snap = snapshot(state)
            for j in range(len(items)):
                a, z = rec['cube_off'][j], rec['cube_off'][j + 1]
                b, y = snap['cube_off'][j], snap['cube_off'][j + 1]
                if z > a:
                    out[j].append(tuple(rec[k][a:z].tobytes() for k in RECORDS[1:5]) + (rows(rec['bits_out'][a:z]), rows(rec['closed_out'][a:z]),
                                  int(rec['first'][j]), snap['len'][b:y].tobytes(), rows(snap['bits'][b:y]), rows(snap['closed'][b:y]),
                                  snap['model'][v0[j]:v0[j + 1]].tobytes(), int(snap['work'][j]), int(snap['status'][j]), int(snap['rounds'][j])))
        return out

    a = trace(p, inst, hints)
    assert sum(len(r) for r in a) > len(inst) + 100 and max(len(r) for r in a) >= 5      # many instances run several rounds
    assert a == trace(p, inst, hints)                                                     # a second run on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    shuffled = [inst[i] for i in order]
    assert [a[i] for i in order] == trace(problem(shuffled), shuffled, [hints[i] for i in order])        # a shuffled batch
    for i in list(range(0, len(inst), 97)) + [len(inst) - 3, len(inst) - 1]:             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            assert [a[i]] == trace(problem([inst[i]]), [inst[i]], [hints[i]])
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every cube, one after the other
    one = trace(p, inst, hints)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    assert a == one
    state = p.exact_solve_begin()
    p.exact_solve_round(state, budget, give)
    assert p.exact_last_grid() > 1
    prev = native.use_build('fast')
    try:
        fast = trace(problem(inst), inst, hints)
    finally:
        native.use_build(prev)
    assert a == fast


def test_hbm_route_keeps_one_cube():
    big = cs.past_the_slab()
    few = cs.family()[:40]
    inst = widen(few[:20] + [big] + few[20:])
    W = words_of(inst)
    # one node a round: the small instances are cut up, the large one keeps its one cube
    mstate = sm.State(inst)
    trace = [model_snapshot(inst, mstate, W)]
    while mstate.cubes():
        trace.append((1, 4) + model_round(inst, mstate, 1, 4, W, whole={20}))
    p = problem(inst)
    state, history = in_lockstep(inst, p, None, trace)
    mine = [h for h in history if h['cube_off'][21] > h['cube_off'][20]]
    assert len(mine) >= 3 and all(h['cube_off'][21] - h['cube_off'][20] == 1 for h in mine)          # several rounds, never expanded
    assert any(h['cube_off'][20] > 20 for h in history)                                   # while the instances before it were
    got = snapshot(state)
    assert got['status'][20] == 1 and satisfied(inst, got['model'])[20] and got['rounds'][20] == len(mine)
    plain = [t.cpu().numpy() for t in p.exact_solve()]
    assert np.array_equal(got['status'], plain[0])
    v0 = sum(n for n, _ in inst[:20])
    assert np.array_equal(got['model'][v0:v0 + inst[20][0]], plain[1][v0:v0 + inst[20][0]])           # one cube: the plain search's model
    # two cubes on the HBM route are refused: its working arrays are per instance
    from pdp import native
    bad = p.exact_solve_begin()
    bad.cube_off[21:] += 1
    for f in ('len', 'bits', 'closed'):
        t = getattr(bad, f)
        setattr(bad, f, torch.cat([t[:21], t[20:21], t[21:]]).contiguous())
    with pytest.raises(native.NativeError, match='instance 20 is on the HBM route'):
        p.exact_solve_round(bad, 1, 0)


def test_too_many_variables_in_a_batch():
    from pdp import native
    few = widen(cs.family()[:6])
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    edge = (1023, [[1, 2], [-1, 1023]])
    inst = few[:3] + [wide] + few[3:] + [edge]
    W = words_of(inst)
    mstate = sm.State(inst)
    trace = [model_snapshot(inst, mstate, W)]
    while mstate.cubes():
        trace.append((30, 2) + model_round(inst, mstate, 30, 2, W))
    p = problem(inst)
    state, history = in_lockstep(inst, p, None, trace)
    got = snapshot(state)
    assert got['status'][3] == -2 and got['status'][7] == 1 and got['bits'].shape == (0, 32)
    assert (got['work'][3], got['rounds'][3]) == (0, 0) and not got['model'][sum(n for n, _ in inst[:3]):][:1024].any()
    assert all(h['first'][3] == -1 for h in history)
    assert history[0]['cube_off'].tolist() == [0, 1, 2, 3, 3, 4, 5, 6, 7]                 # no cube on the wide instance
    bad = p.exact_solve_begin()
    bad.cube_off[4:] += 1
    for f in ('len', 'bits', 'closed'):
        t = getattr(bad, f)
        setattr(bad, f, torch.cat([t[:1], t]).contiguous())
    with pytest.raises(native.NativeError, match='cube 3 is on an instance of more than 1023 variables'):
        p.exact_solve_round(bad, 1, 0)
    # the driver sends the wide instance to the plain call
    from pdp import exact
    st, models, work = exact.solve_items([exact.raw_item(n, c) for n, c in inst], split='rounds', round_budget=30)
    assert st.tolist() == [int(s) if s != -2 else 1 for s in got['status']] and work[3] > 0
    assert all((any((models[3][abs(l) - 1] > 0.5) == (l > 0) for l in c)) for c in wide[1])


def test_a_state_continues_on_another_problem(batch):
    inst, p, plain = batch
    hints = flat_hints(inst, hints_for(True))
    state = p.exact_solve_begin(hints)
    for _ in range(3):
        assert p.exact_solve_round(state, 200, 2) > 0
    held = state.cpu()
    assert all(getattr(held, f).device.type == 'cpu' for f in held.FIELDS) and held.cubes == state.cubes
    before = snapshot(state)
    q = problem(inst)                                                                     # a new handle of the same items
    moved = held.to(q.device)
    rounds = 0
    while moved.cubes:
        q.exact_solve_round(moved, 5000, 1)
        p.exact_solve_round(state, 5000, 1)
        rounds += 1
    same(snapshot(moved), snapshot(state), 'continued')
    same(snapshot(held), before, 'the copy is left alone')
    got = snapshot(moved)
    assert np.array_equal(got['status'], plain[True][0]) and satisfied(inst, got['model'])[got['status'] == 1].all()
    assert rounds >= 2


def test_caller_made_frontier_of_closed_paths(batch):
    # all 2^d closed paths of depth d on one instance are pdp_exact_solve_split's cubes: together they decide as the instance does
    # (where the tree is shallower than the path, as in the small instance here, a model is met inside the path)
    inst, p, plain = batch
    st = plain[False][0]
    v0 = np.concatenate([[0], np.cumsum([n for n, _ in inst])])
    small = next(j for j, (n, _) in enumerate(inst) if 5 <= n <= 8 and st[j] == 1)
    unsat = next(j for j in range(len(inst) - 1, 0, -1) if st[j] == 0)
    d = 5
    for j in (small, unsat, len(inst) - 5):
        for f_budget in (0, 300):
            state = p.exact_solve_begin()
            ln, bits, closed = sm.pack([[((i >> (d - 1 - k)) & 1, 1) for k in range(d)] for i in range(1 << d)], state.bits.size(1))
            off = np.zeros(len(inst) + 1, dtype=np.int64)
            off[j + 1:] = 1 << d
            state.cube_off, state.len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
            state.bits, state.closed = torch.from_numpy(bits).cuda(), torch.from_numpy(closed).cuda()
            while state.cubes:
                p.exact_solve_round(state, f_budget, 1)
            got = snapshot(state)
            assert got['status'][j] == st[j] and (got['status'][np.arange(len(inst)) != j] < 0).all()
            assert st[j] == 0 or satisfied([inst[j]], got['model'][v0[j]:v0[j + 1]])[0]
            assert not np.delete(got['model'], np.arange(v0[j], v0[j + 1])).any()


def test_refusals_write_nothing(batch):
    from pdp import native
    from pdp.factorgraph import dataset
    inst, p, _ = batch
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    r2 = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        r2.exact_solve_begin()
    L = native.lib()
    one = torch.zeros(8, dtype=torch.int64, device=p.device)
    assert L.pdp_exact_solve_round(r2._h, None, native.ptr(one), ctypes.c_int64(0), None, None, None, ctypes.c_int64(1), native.ptr(one),
                                   native.ptr(one), native.ptr(one), native.ptr(one), None, None, None, None, None, None, None) == 4
    good = p.exact_solve_begin()
    p.exact_solve_round(good, 1, 2)
    p.exact_solve_round(good, 1, 2)
    assert good.cubes > 50
    base = snapshot(good)

    def broken(field, at, value):
        s = good.to(p.device)
        getattr(s, field).view(-1)[at] = value
        return s

    W = good.bits.size(1)
    c = int(np.nonzero(base['len'] >= 2)[0][-1])
    owner = int(np.searchsorted(base['cube_off'], c, side='right')) - 1
    negative = broken('len', c, -1)
    pair = broken('closed', c * W, int(base['closed'][c, 0]) & ~3 | 1)                    # level 2 of cube c: not closed,
    pair.bits.view(-1)[c * W] = int(base['bits'][c, 0]) | 2                               # and on its other polarity: the pair (1, 0)
    cases = [(broken('cube_off', 0, 1), 'cube_off must start at 0.*instance 0'),
             (broken('cube_off', 7, int(base['cube_off'][8]) + 1), 'cube_off must start at 0, never fall.*instance 7'),
             (broken('cube_off', len(inst), int(base['cube_off'][-1]) - 1), r'cube_off must start at 0.*instance %d' % (len(inst) - 1)),
             (negative, 'length of cube %d is not in 0' % c),
             (broken('len', c, 1 << 20), 'length of cube %d is not in 0' % c),
             (broken('len', c, inst[owner][0] + 1), 'length of cube %d is not in 0' % c),
             (pair, r'cube %d has a level on its other polarity that is not closed' % c)]
    for s, said in cases:
        before = snapshot(s)
        with pytest.raises(native.NativeError, match=said) as e:
            p.exact_solve_round(s, 1, 1)
        assert 'pdp_exact_solve_round: ' in str(e.value)
        same(snapshot(s), before, said)                                                   # answers and frontier as they were
    # the Python layer: the state's tensors, the hints, the budget and give
    for field, wrong in (('len', good.len.to(torch.int64)), ('bits', good.bits[:, :0]), ('model', good.model.cpu()), ('work', good.work[:-1]),
                         ('hint', good.hint.to(torch.float64)), ('status', good.status.to(torch.int32))):
        s = good.to(p.device)
        setattr(s, field, wrong)
        with pytest.raises(native.NativeError, match='state.%s must be' % field):
            p.exact_solve_round(s)
    for kw in (dict(budget=1.5), dict(budget=True), dict(give=-1), dict(give='2'), dict(give=1024)):
        with pytest.raises(ValueError):
            p.exact_solve_round(good, **kw)
    with pytest.raises(ValueError):
        p.exact_solve_round(p.exact_count_begin())
    for wrong in (good.hint[:-1], good.hint.cpu(), good.hint.to(torch.float64), [0.5] * p.V):
        with pytest.raises(ValueError, match='hints must be'):
            p.exact_solve_begin(wrong)
    outs = [torch.full((good.cubes,), -7, dtype=torch.int8, device=p.device), torch.full((good.cubes,), -7, dtype=torch.int32, device=p.device),
            torch.full((good.cubes, W), -7, dtype=torch.int32, device=p.device), torch.full((good.cubes, W), -7, dtype=torch.int32, device=p.device)]
    first = torch.full((p.B,), -7, dtype=torch.int32, device=p.device)
    too_many = L.pdp_exact_solve_round(p._h, native.ptr(good.hint), native.ptr(good.cube_off), ctypes.c_int64((1 << 22) + 1), native.ptr(good.len),
                                       native.ptr(good.bits), native.ptr(good.closed), ctypes.c_int64(1), native.ptr(good.status),
                                       native.ptr(good.model), native.ptr(good.work), native.ptr(first), *[native.ptr(t) for t in outs], None, None,
                                       None)
    assert too_many != native.PDP_OK and b'a frontier holds 0 .. 2^22' in L.pdp_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs + [first])
    same(snapshot(good), base, 'the good state')


def test_solve_items_rounds_on_segments_and_items_without_a_literal():
    from pdp import exact
    inst = cs.family()[:120] + cs.uniform_3sat(150, 30, (4.0, 4.3, 5.0), 3)
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + [exact.raw_item(4, [[]])]
    rng = np.random.RandomState(3)
    hints = [None if j % 4 == 0 else rng.rand(int(it[0])).astype(np.float32) for j, it in enumerate(raw)]
    base = exact.solve_items(raw, hints=hints)
    assert set(base[0].tolist()) == {0, 1} and (base[0][-10:-1] == 0).sum() >= 3

    def sat(item, model):
        n, m, gm, ef = item[:4]
        ok = np.zeros(m, dtype=bool)
        np.logical_or.at(ok, gm[1], (model[gm[0]] > 0.5) == (ef > 0))
        return bool(ok.all())

    for max_edges in (exact.MAX_EDGES, 400):
        got = exact.solve_items(raw, hints=hints, split='rounds', round_budget=2000, max_edges=max_edges)
        assert len(got) == 3 and np.array_equal(got[0], base[0]) and (got[0].dtype, got[2].dtype) == (np.int8, np.int64)
        for it, s, m, bm in zip(raw, got[0], got[1], base[1]):
            assert m.dtype == np.float32 and m.shape == bm.shape and (sat(it, m) if s == 1 else not m.any())
        assert got[2][0] == got[2][1] == got[2][-1] == 0 and (got[2][-10:-1] >= base[2][-10:-1]).all()
    assert exact.label_clause_lists(inst[-9:], split='rounds', round_budget=2000) == [bool(s) for s in base[0][-10:-1]]
    assert exact.is_sat(*inst[-1], split='rounds') == bool(base[0][-2])
    # a total budget: the instances that reach it end undecided, the others as before
    total = int(np.median(base[2][-10:-1]))
    low = exact.solve_items(raw, hints=hints, budget=total, split='rounds', round_budget=500)
    out = low[0] == -1
    assert out.sum() >= 2 and np.array_equal(low[0][~out], base[0][~out]) and (low[2][out] >= total).all()
    assert all(not m.any() for m, o in zip(low[1], out) if o)
    few = exact.solve_items(raw, hints=hints, split='rounds', round_budget=100, rounds=2)
    assert (few[0] == -1).sum() >= 5 and np.array_equal(few[0][few[0] != -1], base[0][few[0] != -1])


def test_cli_complete_rounds(tmp_path):
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    clauses_of = []
    for i in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 128)
        clauses_of.append(clauses)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-rounds', '10'], 1, str(tmp_path / 'deep.jsonl'), 0)
    assert len(base) == len(deep) == 40
    several = 0
    by_id = {}
    for b, d in zip(base, deep):
        r, rb = json.loads(d), json.loads(b)
        assert 'complete_rounds' not in rb
        keys = list(rb)
        keys.insert(keys.index('work') + 1, 'complete_rounds')
        assert list(r) == keys                                                            # "complete_rounds" right after "work"
        assert r['complete'] == rb['complete'] in (0, 1) and r['complete_rounds'] >= 1
        free = ('work', 'complete_rounds', 'solution')
        assert {k: v for k, v in r.items() if k not in free} == {k: v for k, v in rb.items() if k not in free}
        if r['complete'] == 1:
            by_id[r['ID']] = r['solution']
            assert r['solved'] == 1 and r['unsat_clauses'] == 0
        several += r['complete_rounds'] > 1
    assert several >= 5 and len(by_id) >= 5
    # every solution of a rounds row is a model of its file
    hits = 0
    for i, clauses in enumerate(clauses_of):
        for s in [s for k, s in by_id.items() if 't_%02d_0' % i in str(k)]:
            assert all(any((s[abs(l) - 1] > 0.5) == (l > 0) for l in c) for c in clauses)
            hits += 1
    assert hits == len(by_id)
