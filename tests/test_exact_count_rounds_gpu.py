"""The resumable counting search on the GPU (pdp_exact_count_round, pdp_exact_count_expand, Problem.exact_count_begin / exact_count_round,
exact.count_models(split='rounds'), satyr.py --complete --complete-count --complete-count-rounds): equal to its Python statement
(tests/exact_count_rounds_model.py) bit for bit, round by round, in the totals, every cube record, every checkpoint and every word of the
expanded frontier; completed counts equal to exact_count; the work bound of a round; determinism over call, batch, grid and build; the HBM
route and instances that are too large; a state continued on another handle; refusals with nothing written; the host entry points; the
command line."""
import ctypes
import faulthandler
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_count_model as cm
import exact_count_rounds_model as rm
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
PAIRS = [(1, 0), (1, 3), (40, 1), (200, 8), (3000, 2)]  # reads per cube and round, levels given away; the last one runs several nodes a round
RECORDS = ('cube_off', 'cube_status', 'cube_count', 'cube_work', 'cube_leaves', 'cube_replay', 'len_out', 'bits_out', 'closed_out')
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
    return [(rm.inst_n(i), i[1]) for i in inst]


def snapshot(state):
    "every tensor of a CountState as numpy"
    return {f: getattr(state, f).cpu().numpy() for f in state.FIELDS}


def one_round(p, state, budget, give):
    "Problem.exact_count_round(stats=True): (open cubes, the records as a dict of numpy arrays)"
    made, rec = p.exact_count_round(state, budget, give, stats=True)
    rec = dict(zip(RECORDS, [t.cpu().numpy() for t in rec]))
    assert [rec[k].dtype for k in RECORDS] == [np.int64, np.int8, np.float64, np.int64, np.int64, np.int64, np.int32, np.int32, np.int32]
    assert made == state.cubes == int(state.cube_off[-1].item())
    return made, rec


def model_round(inst, mstate, budget, give, W, whole=()):
    "one round of the model in the layout of one_round's records, and the State's totals and frontier in snapshot's"
    ran = rm.frontier(mstate, W)[0]
    rec = rm.round(inst, mstate, budget, give, whole)
    ln, bits, closed = rm.pack([r[6] or [] for r in rec], W)
    want = dict(cube_off=ran, cube_status=np.array([r[1] for r in rec], dtype=np.int8), cube_count=np.array([r[2] for r in rec], dtype=np.float64),
                cube_work=np.array([r[3] for r in rec], dtype=np.int64), cube_leaves=np.array([r[4] for r in rec], dtype=np.int64),
                cube_replay=np.array([r[5] for r in rec], dtype=np.int64), len_out=ln, bits_out=bits, closed_out=closed)
    return want, model_snapshot(mstate, W)


def model_snapshot(mstate, W):
    off, ln, bits, closed = rm.frontier(mstate, W)
    return dict(cube_off=off, len=ln, bits=bits, closed=closed, count=np.array(mstate.count, dtype=np.float64),
                true_count=np.concatenate(mstate.true_count), work=np.array(mstate.work, dtype=np.int64),
                leaves=np.array(mstate.leaves, dtype=np.int64), status=np.array(mstate.status(), dtype=np.int8),
                rounds=np.array(mstate.rounds, dtype=np.int32))


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def in_lockstep(inst, p, budget, give, whole=(), max_rounds=1 << 20):
    "the GPU and the model, round by round until the frontier is empty: every record, total and frontier word equal; the per-round records"
    W = rm.words(max([n for n, _ in inst if n <= rm.MAX_N] + [0]))
    state, mstate = p.exact_count_begin(), rm.State(inst)
    same(snapshot(state), model_snapshot(mstate, W), 'begin')
    history = []
    schedule = budget if callable(budget) else (lambda r: budget)
    while mstate.cubes() and len(history) < max_rounds:
        budget = schedule(len(history))
        made, rec = one_round(p, state, budget, give)
        want, after = model_round(inst, mstate, budget, give, W, whole)
        same(rec, want, 'records of round %d' % len(history))
        same(snapshot(state), after, 'state after round %d' % len(history))
        assert made == mstate.cubes()
        history.append(rec)
    return state, history


@pytest.fixture(scope='module')
def batch():
    """about 420 instances in one problem: the host family (n <= 12), the two fans, uniform 3-SAT of n = 20 at ratio 3.5 and n = 30 at 4.0;
    the plain count of the same handle, computed once"""
    few = cs.family()
    inst = widen(few + [cs.fan(k) for k in cs.FAN_K] + cs.uniform_3sat(20, 20, (3.5,), 2) + cs.uniform_3sat(30, 30, (4.0,), 2))
    p = problem(inst)
    plain = [t.cpu().numpy() for t in p.exact_count(stats=True)]
    return inst, p, plain


def finished(state, plain, sure=None):
    "a completed state against exact_count's (status, count, true_count, work, leaves) of the same handle"
    got = snapshot(state)
    assert got['cube_off'].tolist() == [0] * len(got['cube_off']) and got['len'].shape == (0,)
    sure = np.ones(len(plain[0]), dtype=bool) if sure is None else sure
    assert np.array_equal(got['status'], plain[0])
    assert np.array_equal(got['count'][sure], plain[1][sure]) and np.array_equal(got['leaves'][sure], plain[4][sure])
    assert (got['work'] >= plain[3]).all()
    return got


@pytest.mark.parametrize('budget,give', PAIRS)
def test_equal_to_the_python_model_round_by_round(batch, budget, give):
    from pdp import exact
    inst, p, plain = batch
    assert len(inst) >= 415
    state, history = in_lockstep(inst, p, budget, give)
    print('rounds budget %d give %d: %d rounds, frontier peak %d cubes, reads %.2f times the plain count'
          % (budget, give, len(history), max(len(h['cube_status']) for h in history), state.work.sum().item() / plain[3].sum()))
    sure = exact.count_is_exact(plain[0], plain[1])
    got = finished(state, plain, sure)
    few = len(cs.family())
    assert sure[:few].all() and not sure[few + 1] and (plain[0] == 1).all()                # 2^150 + 1 is not exact
    tc, pt = np.split(got['true_count'], np.cumsum([n for n, _ in inst])[:-1]), np.split(plain[2], np.cumsum([n for n, _ in inst])[:-1])
    assert all(np.array_equal(a, b) for a, b, s in zip(tc, pt, sure) if s)
    for j, (bc, bt) in enumerate(cs.family_brute()):                                      # brute force for the n <= 12 part
        assert got['count'][j] == bc and tc[j].tolist() == bt.tolist()
    for j, k in enumerate(cs.FAN_K):                                                      # 150 forced variables on one level: three chunks of lanes
        assert got['count'][few + j] >= 2.0 ** k and got['leaves'][few + j] == 2
    assert (len(history) > 100) == ((budget, give) == (1, 0)) and got['rounds'].max() == len(history)
    # the work bound of a round: the replay, the budget, and one node (at most n + 1 passes of e reads and a branching pass of 2 e)
    node = np.array([(n + 3) * sum(len(c) for c in cl) for n, cl in inst], dtype=np.int64)
    stopped = 0
    for h in history:
        per = np.repeat(node, np.diff(h['cube_off']))
        assert (h['cube_replay'] <= h['cube_work']).all() and (h['cube_work'] <= h['cube_replay'] + budget + per).all()
        assert (h['cube_work'][h['cube_status'] == -1] - h['cube_replay'][h['cube_status'] == -1] >= budget).all()
        assert (h['len_out'][h['cube_status'] == 1] == 0).all() and set(h['cube_status'].tolist()) <= {-1, 1}
        stopped += int((h['cube_status'] == -1).sum())
    assert stopped >= 20
    if give:
        assert max(int(np.diff(h['cube_off']).max()) for h in history) > give             # an instance's frontier grew past one expansion


def test_deterministic_in_every_output_and_frontier_word(batch, monkeypatch):
    from pdp import native
    inst, p, _ = batch
    budget, give = 40, 2

    def rows(words):
        "the rows of a path array as integers, whatever the words per row: a lone instance has narrower rows than the batch"
        return tuple(sum(int(x) << (32 * k) for k, x in enumerate(r)) for r in words.view(np.uint32))

    def trace(prob, items):
        """every record and every state of a run, per instance and round, in a comparable form; an instance's rows end with the round it
        ended in (later rounds repeat its totals)"""
        state, out = prob.exact_count_begin(), [[] for _ in items]
        v0 = np.concatenate([[0], np.cumsum([n for n, _ in items])])
        while state.cubes:
            _, rec = one_round(prob, state, budget, give)
            snap = snapshot(state)
            for j in range(len(items)):
                a, z = rec['cube_off'][j], rec['cube_off'][j + 1]
                b, y = snap['cube_off'][j], snap['cube_off'][j + 1]
                if z > a:
                    out[j].append(tuple(rec[k][a:z].tobytes() for k in RECORDS[1:7]) + (rows(rec['bits_out'][a:z]), rows(rec['closed_out'][a:z]),
                                  snap['len'][b:y].tobytes(), rows(snap['bits'][b:y]), rows(snap['closed'][b:y]), snap['count'][j].tobytes(),
                                  snap['true_count'][v0[j]:v0[j + 1]].tobytes(), int(snap['work'][j]), int(snap['leaves'][j]),
                                  int(snap['status'][j]), int(snap['rounds'][j])))
        return out

    a = trace(p, inst)
    assert sum(len(r) for r in a) > 2 * len(inst)
    assert a == trace(p, inst)                                                            # a second run on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    shuffled = [inst[i] for i in order]
    assert [a[i] for i in order] == trace(problem(shuffled), shuffled)                    # a shuffled batch
    for i in list(range(0, len(inst), 97)) + [len(inst) - 3, len(inst) - 1]:             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            assert [a[i]] == trace(problem([inst[i]]), [inst[i]])
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every cube, one after the other
    one = trace(p, inst)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    assert a == one
    state = p.exact_count_begin()
    p.exact_count_round(state, budget, give)
    assert p.exact_last_grid() > 1
    prev = native.use_build('fast')
    try:
        fast = trace(problem(inst), inst)
    finally:
        native.use_build(prev)
    assert a == fast


def test_hbm_route_keeps_one_cube():
    big = cs.past_the_slab()
    few = cs.family()[:40]
    inst = widen(few[:20] + [big] + few[20:])
    p = problem(inst)
    want = cs.slab_result()
    # two rounds of one node each, in which the small instances are cut up, then several rounds of a sixth of the large one's reads
    state, history = in_lockstep(inst, p, lambda r: 1 if r < 2 else want[3] // 6, 4, whole={20})
    assert len(history) >= 5
    for h in history:
        assert h['cube_off'][21] - h['cube_off'][20] == 1                                 # never expanded, open to the last round
    assert history[2]['cube_off'][20] > 20                                                # while the instances before it were
    got = snapshot(state)
    assert (got['status'][20], got['count'][20], got['leaves'][20]) == (1, want[1], want[4]) and got['work'][20] >= want[3]
    assert np.array_equal(got['true_count'][sum(n for n, _ in inst[:20]):][:inst[20][0]], want[2])
    brute = cs.family_brute()[:40]
    rest = [i for i in range(len(inst)) if i != 20]
    assert [got['count'][i] for i in rest] == [b[0] for b in brute]
    # two cubes on the HBM route are refused: its working arrays are per instance
    from pdp import native
    bad = p.exact_count_begin()
    bad.cube_off[21:] += 1
    for f in ('len', 'bits', 'closed'):
        t = getattr(bad, f)
        setattr(bad, f, torch.cat([t[:21], t[20:21], t[21:]]).contiguous())
    with pytest.raises(native.NativeError, match='instance 20 is on the HBM route'):
        p.exact_count_round(bad, 1, 0)


def test_too_many_variables_in_a_batch():
    from pdp import native
    few = widen(cs.family()[:6])
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    edge = (1023, [[1, 2], [-1, 1023]])
    inst = few[:3] + [wide] + few[3:] + [edge]
    p = problem(inst)
    state, history = in_lockstep(inst, p, 30, 2)
    got = snapshot(state)
    assert got['status'].tolist() == [1, 1, 1, -2, 1, 1, 1, 1] and got['bits'].shape == (0, 32)
    assert (got['count'][3], got['work'][3], got['leaves'][3], got['rounds'][3]) == (0.0, 0, 0, 0)
    assert got['count'][7] == 2.0 ** 1022 and np.isfinite(got['true_count']).all()
    assert history[0]['cube_off'].tolist() == [0, 1, 2, 3, 3, 4, 5, 6, 7]                 # no cube on the wide instance
    bad = p.exact_count_begin()
    bad.cube_off[4:] += 1
    for f in ('len', 'bits', 'closed'):
        t = getattr(bad, f)
        setattr(bad, f, torch.cat([t[:1], t]).contiguous())
    with pytest.raises(native.NativeError, match='cube 3 is on an instance of more than 1023 variables'):
        p.exact_count_round(bad, 1, 0)


def test_a_state_continues_on_another_problem(batch):
    inst, p, plain = batch
    state = p.exact_count_begin()
    for _ in range(3):
        assert p.exact_count_round(state, 200, 2) > 0
    held = state.cpu()
    assert all(getattr(held, f).device.type == 'cpu' for f in held.FIELDS) and held.cubes == state.cubes
    before = snapshot(state)
    q = problem(inst)                                                                     # a new handle of the same items
    moved = held.to(q.device)
    rounds = 0
    while moved.cubes:
        q.exact_count_round(moved, 5000, 1)
        p.exact_count_round(state, 5000, 1)
        rounds += 1
    same(snapshot(moved), snapshot(state), 'continued')
    same(snapshot(held), before, 'the copy is left alone')
    from pdp import exact
    finished(moved, plain, exact.count_is_exact(plain[0], plain[1]))
    assert rounds >= 2


def test_caller_made_frontier_of_closed_paths(batch):
    # all 2^d closed paths of depth d on one instance are pdp_exact_count_split's cubes: they sum to the count
    # (where the tree is shallower than the path, as in the small instance here, a leaf is met inside the path and counted by one of them)
    inst, p, plain = batch
    v0 = np.concatenate([[0], np.cumsum([n for n, _ in inst])])
    small = next(j for j, (n, _) in enumerate(inst) if 5 <= n <= 8 and plain[4][j] >= 3)
    d = 5
    for j in (small, len(inst) - 1):
        for f_budget in (0, 300):
            state = p.exact_count_begin()
            ln, bits, closed = rm.pack([[((i >> (d - 1 - k)) & 1, 1) for k in range(d)] for i in range(1 << d)], state.bits.size(1))
            off = np.zeros(len(inst) + 1, dtype=np.int64)
            off[j + 1:] = 1 << d
            state.cube_off, state.len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
            state.bits, state.closed = torch.from_numpy(bits).cuda(), torch.from_numpy(closed).cuda()
            while state.cubes:
                p.exact_count_round(state, f_budget, 1)
            got = snapshot(state)
            assert (got['count'][j], got['leaves'][j]) == (plain[1][j], plain[4][j]) and got['count'].sum() == plain[1][j] > 0
            assert np.array_equal(got['true_count'][v0[j]:v0[j + 1]], plain[2][v0[j]:v0[j + 1]])


def test_refusals_write_nothing(batch, tmp_path):
    from pdp import native
    from pdp.factorgraph import dataset
    inst, p, _ = batch
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    r2 = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        r2.exact_count_begin()
    good = p.exact_count_begin()
    p.exact_count_round(good, 1, 2)
    p.exact_count_round(good, 1, 2)
    assert good.cubes > len(inst)
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
    assert p.exact_count_round(broken('len', c, inst[owner][0]), 1, 0) >= 0               # a path of n levels is allowed
    for s, said in cases:
        before = snapshot(s)
        with pytest.raises(native.NativeError, match=said):
            p.exact_count_round(s, 1, 1)
        same(snapshot(s), before, said)                                                   # totals and frontier as they were
    # the expansion checks what it is given as well, and refuses a frontier past its capacity; nothing is written then
    L = native.lib()
    cube_status = torch.full((good.cubes,), -1, dtype=torch.int8, device=p.device)
    out = [torch.full((p.B + 1,), -7, dtype=torch.int64, device=p.device), torch.full((good.cubes,), -7, dtype=torch.int32, device=p.device),
           torch.full((good.cubes, W), -7, dtype=torch.int32, device=p.device), torch.full((good.cubes, W), -7, dtype=torch.int32, device=p.device)]
    made = ctypes.c_int64(-7)

    def expand(s, give, capacity):
        return L.pdp_exact_count_expand(p._h, native.ptr(s.cube_off), ctypes.c_int64(s.cubes), native.ptr(cube_status), native.ptr(s.len),
                                        native.ptr(s.bits), native.ptr(s.closed), ctypes.c_int32(give), ctypes.c_int64(capacity),
                                        *[native.ptr(t) for t in out], ctypes.byref(made), None)

    assert expand(good, 1, good.cubes - 1) != native.PDP_OK and b'more than the capacity' in L.pdp_last_error()
    assert expand(negative, 0, good.cubes) != native.PDP_OK and b'length of cube' in L.pdp_last_error()
    assert expand(good, -1, good.cubes) != native.PDP_OK
    torch.cuda.synchronize()
    assert made.value == -7 and all(bool((t == -7).all()) for t in out)
    assert expand(good, 0, good.cubes) == native.PDP_OK and made.value == good.cubes      # every cube "stopped", nothing given: as it was
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), base['cube_off']) and np.array_equal(out[1].cpu().numpy(), base['len'])
    assert np.array_equal(out[2].cpu().numpy(), base['bits']) and np.array_equal(out[3].cpu().numpy(), base['closed'])
    # the Python layer: the state's tensors, the budget and give
    for field, wrong in (('len', good.len.to(torch.int64)), ('bits', good.bits[:, :0]), ('count', good.count.cpu()), ('work', good.work[:-1])):
        s = good.to(p.device)
        setattr(s, field, wrong)
        with pytest.raises(native.NativeError, match='state.%s must be' % field):
            p.exact_count_round(s)
    for kw in (dict(budget=1.5), dict(budget=True), dict(give=-1), dict(give='2'), dict(give=1024)):
        with pytest.raises(ValueError):
            p.exact_count_round(good, **kw)
    with pytest.raises(ValueError):
        p.exact_count_round(snapshot(good))
    outs = [torch.full((good.cubes,), -7, dtype=torch.int8, device=p.device), out[1], out[2], out[3]]
    for t in out[1:]:
        t.fill_(-7)
    too_many = L.pdp_exact_count_round(p._h, native.ptr(good.cube_off), ctypes.c_int64((1 << 22) + 1), native.ptr(good.len), native.ptr(good.bits),
                                       native.ptr(good.closed), ctypes.c_int64(1), native.ptr(good.count), native.ptr(good.true_count),
                                       native.ptr(good.work), native.ptr(good.leaves), *[native.ptr(t) for t in outs], None, None, None, None, None)
    assert too_many != native.PDP_OK and b'a frontier holds 0 .. 2^22' in L.pdp_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs)
    same(snapshot(good), base, 'the good state')
    for argv, said in ((['--complete', '--complete-count-rounds', '3'], 'give --complete-count as well'),
                       (['--complete', '--complete-count', '--complete-count-rounds', '41'], 'from 0 to 40'),
                       (['--complete', '--complete-count', '--complete-count-rounds', '3', '--complete-count-split', '2'],
                        'without --complete-count-split')):
        r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d'] + argv +
                           ['-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                           cwd=REPO)
        assert r.returncode != 0 and '--complete-count-rounds' in r.stderr and said in r.stderr


def test_count_models_rounds_on_segments_and_items_without_a_literal():
    from pdp import exact
    inst = cs.family()[:120] + cs.uniform_3sat(150, 30, (3.5, 4.26, 5.0), 3)
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + \
        [exact.raw_item(4, [[]]), exact.raw_item(1024, []), exact.raw_item(1024, [[1, 2], [-1, 1024]])]
    base = exact.count_models(raw)
    assert set(base[0].tolist()) == {-2, 1} and exact.count_is_exact(base[0], base[1])[:-2].all()
    for max_edges in (exact.MAX_EDGES, 400):
        got = exact.count_models(raw, split='rounds', round_budget=2000, max_edges=max_edges, depths=True)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        assert (got[0].dtype, got[1].dtype, got[3].dtype, got[4].dtype) == (np.int8, np.float64, np.int64, np.int32)
        for a, b in zip(got[2], base[2]):
            assert (a is None) == (b is None) and (a is None or (a.dtype == np.float64 and np.array_equal(a, b)))
        assert (got[3] >= base[3]).all() and got[3][0] == got[3][1] == got[3][-3] == got[3][-2] == got[3][-1] == 0
        assert got[4][-2] == got[4][-1] == 0 and got[4].max() >= 2 and (got[4][-12:-3] >= 1).all()      # no cube: no round
    assert len(exact.count_models(raw[:5], split='rounds')) == 4
    # a total budget: the instances that reach it end with a lower bound, the others as before
    total = int(np.median(base[3][-12:-3]))
    low = exact.count_models(raw, budget=total, split='rounds', round_budget=500, depths=True)
    out = low[0] == -1
    assert out.sum() >= 3 and (low[0][~out] == base[0][~out]).all() and np.array_equal(low[1][~out], base[1][~out])
    assert (low[1][out] <= base[1][out]).all() and (low[3][out] >= total).all() and (base[3][out] > total // 64).all()
    few = exact.count_models(raw, split='rounds', round_budget=100, rounds=2, depths=True)
    assert few[4].max() == 2 and (few[0] == -1).sum() >= 5 and (few[1] <= base[1]).all()


def test_cli_complete_count_rounds(tmp_path):
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    for i in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 128)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete', '--complete-count']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-count-rounds', '10'], 1, str(tmp_path / 'deep.jsonl'), 0)
    auto, _ = _run(argv + ['--complete-count-rounds', '-1'], 1, str(tmp_path / 'auto.jsonl'), 0)
    assert len(base) == len(deep) == len(auto) == 40
    counted = 0
    for b, d, a in zip(base, deep, auto):
        r, rb, ra = json.loads(d), json.loads(b), json.loads(a)
        if 'count_rounds' not in r:
            assert d == b == a and rb['complete'] != 1                                    # byte-identical to the run without the flag
            continue
        assert list(r)[-2:] == ['count_work', 'count_rounds'] and list(r)[:-1] == list(rb) and list(ra) == list(r)
        assert {k: v for k, v in r.items() if k not in ('count_work', 'count_rounds')} == {k: v for k, v in rb.items() if k != 'count_work'}
        assert {k: v for k, v in ra.items() if k not in ('count_work', 'count_rounds')} == {k: v for k, v in rb.items() if k != 'count_work'}
        assert r['count_work'] >= rb['count_work'] and rb['model_count_proved'] == 1 and r['count_rounds'] >= ra['count_rounds'] >= 1
        counted += 1
    assert counted >= 5
