"""The split optimising search on the GPU (pdp_exact_min_unsat_split, Problem.exact_min_unsat_split, exact.min_unsat(split=), satyr.py
--complete --complete-min-unsat --complete-min-unsat-split).  With one wave (PDP_EXACT_GRID=1) every output and cube record equals the
Python statement's sequential() (tests/exact_min_unsat_split_model.py) bit for bit.  With the full grid only what is promised is compared:
status 1, the cost (against the plain model, exact_min_unsat and pdp_cnf_eval on the same handle), a model that attains it, the cube that
holds it, depth_used.  Depth 0 equal to exact_min_unsat in all five outputs under every budget; the budget per cube; an instance wider
than a wave; the HBM route; a prefix that ends early; determinism of the promised fields; refusals; the host entry point; the command
line.  Which minimiser comes back, first, work, improvements and the records depend on timing above one wave and are not compared."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_min_unsat_cases as cs
import exact_min_unsat_model as mm
import exact_min_unsat_split_cases as sc
import exact_min_unsat_split_model as sm
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
KEYS = ('status', 'cost', 'model', 'work', 'improvements', 'first', 'depth_used', 'cube_off', 'cube_status', 'cube_cost', 'cube_work',
        'cube_improvements')
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


def hint_tensor(p, inst, hints):
    "None: a NULL pointer; an instance without hints gets zeros (the all-false incumbent)"
    if hints is None:
        return None
    flat = [np.zeros(n, dtype=np.float32) if h is None else np.asarray(h, dtype=np.float32) for (n, _), h in zip(inst, hints)]
    return torch.from_numpy(np.concatenate(flat)).to(p.device)


def run(inst, hints, depth, budget=0, prob=None):
    "Problem.exact_min_unsat_split(stats=True) as a dict of numpy arrays, the model cut per instance"
    p = problem(inst) if prob is None else prob
    d = depth if isinstance(depth, int) else torch.from_numpy(np.asarray(depth, dtype=np.int8)).cuda()
    got = dict(zip(KEYS, [t.cpu().numpy() for t in p.exact_min_unsat_split(budget, hints=hint_tensor(p, inst, hints), depth=d, stats=True)]))
    assert [got[k].dtype for k in KEYS] == [np.int8, np.int32, np.float32, np.int64, np.int32, np.int32, np.int8, np.int64, np.int8, np.int32,
                                            np.int64, np.int32]
    assert got['cube_off'][0] == 0 and np.array_equal(np.diff(got['cube_off']), 1 << got['depth_used'].astype(np.int64))
    assert got['cube_status'].shape == got['cube_cost'].shape == got['cube_work'].shape == got['cube_improvements'].shape == (got['cube_off'][-1],)
    got['model'] = np.split(got['model'], np.cumsum([n for n, _ in inst])[:-1])
    return got


def plain(inst, hints, budget=0, prob=None):
    p = problem(inst) if prob is None else prob
    st, cost, model, work, imp = [t.cpu().numpy() for t in p.exact_min_unsat(budget, hints=hint_tensor(p, inst, hints), stats=True)]
    return st, cost, np.split(model, np.cumsum([n for n, _ in inst])[:-1]), work, imp


def same_as_sequential(got, want, depth):
    "every output and every cube record against the model's sequential(), bit for bit"
    depth = [depth] * len(want) if isinstance(depth, int) else depth
    for j, (st, cost, model, work, imp, first, cubes) in enumerate(want):
        assert (got['status'][j], got['cost'][j], got['work'][j], got['improvements'][j], got['first'][j], got['depth_used'][j]) == \
            (st, cost, work, imp, first, depth[j]), j
        assert np.array_equal(got['model'][j], model), j
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        rec = list(zip(got['cube_status'][a:z].tolist(), got['cube_work'][a:z].tolist(), got['cube_cost'][a:z].tolist(),
                       got['cube_improvements'][a:z].tolist()))
        assert rec == [tuple(c) for c in cubes], j


def promised(inst, got, depth=None):
    "what holds at any grid and any budget: the model attains the cost, the cube named by first holds it, the records add up"
    for j, (_, c) in enumerate(inst):
        assert mm.unsat_count(c, got['model'][j]) == got['cost'][j], j
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        f = got['first'][j]
        assert -1 <= f < z - a and (f == -1 or got['cube_cost'][a + f] == got['cost'][j]), j
        held = got['cube_cost'][a:z]
        assert ((held == sm.NO_COST) | (held >= got['cost'][j])).all(), j
        assert got['status'][j] == (1 if (got['cube_status'][a:z] == 1).all() else -1), j
        assert got['improvements'][j] == got['cube_improvements'][a:z].sum(), j
    assert set(np.unique(got['cube_status']).tolist()) <= {-1, 1}
    if depth is not None:
        assert np.array_equal(got['depth_used'], np.asarray(depth, dtype=np.int8))


def proved(inst, got, cost, depth):
    "with a budget that no cube exhausts: status 1 and the minimum, on top of promised()"
    promised(inst, got, depth)
    assert (got['status'] == 1).all() and (got['cube_status'] == 1).all()
    np.testing.assert_array_equal(got['cost'], cost)


@pytest.fixture(scope='module')
def handle():
    return problem(sc.batch()[0])


@pytest.mark.parametrize('kind', sc.KINDS)
def test_one_wave_equals_the_python_model_exactly(handle, kind, monkeypatch):
    inst, hints, depth = sc.batch()
    assert len(inst) >= 135 and set(depth.tolist()) == set(range(7))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    got = run(inst, hints[kind], depth, prob=handle)
    assert handle.exact_last_grid() == 1
    want = sc.batch_sequential(kind)
    print('min_unsat split, %s: %d instances, %d cubes, %d improved, %d cubes with an improvement, work %d'
          % (kind, len(inst), len(got['cube_status']), int((got['improvements'] > 0).sum()), int((got['cube_improvements'] > 0).sum()),
             int(got['work'].sum())))
    same_as_sequential(got, want, depth.tolist())
    proved(inst, got, sc.batch_plain(kind)[1], depth)
    np.testing.assert_array_equal(got['cost'][:len(sc.family_brute())], sc.family_brute())
    assert int((got['improvements'] > 0).sum()) > 30 and int((got['first'] == -1).sum()) > 5


@pytest.mark.parametrize('kind', sc.KINDS)
def test_full_grid_keeps_what_is_promised(handle, kind):
    inst, hints, depth = sc.batch()
    got = run(inst, hints[kind], depth, prob=handle)
    assert handle.exact_last_grid() > 1
    proved(inst, got, sc.batch_plain(kind)[1], depth)
    st, cost = plain(inst, hints[kind], prob=handle)[:2]                                  # exact_min_unsat on the same handle
    assert (st == 1).all()
    np.testing.assert_array_equal(got['cost'], cost)
    ub0 = np.array([mm.unsat_count(c, mm.threshold(n, h)) for (n, c), h in zip(inst, hints[kind])])
    assert (got['cost'] <= ub0).all() and ((got['first'] == -1) == (got['cost'] == ub0)).all()
    # the library's own evaluator: the instances it can take (no empty clause, at least one clause), as a problem of their own
    keep = [i for i, (n, c) in enumerate(inst) if len(c) > 0 and all(len(x) > 0 for x in c)]
    sub = [inst[i] for i in keep]
    p = problem(sub)
    st, cost2, model, _ = p.exact_min_unsat_split(hints=hint_tensor(p, sub, [hints[kind][i] for i in keep]),
                                                  depth=torch.from_numpy(depth[keep]).cuda())
    _, unsat = p.cnf_eval(model)
    np.testing.assert_array_equal(unsat.cpu().numpy().reshape(-1).astype(np.int64), cost2.cpu().numpy().astype(np.int64))
    np.testing.assert_array_equal(cost2.cpu().numpy(), cost[keep])
    np.testing.assert_array_equal(p.exact_min_unsat(hints=hint_tensor(p, sub, [hints[kind][i] for i in keep]))[1].cpu().numpy(), cost[keep])
    assert (st.cpu().numpy() == 1).all()


@pytest.mark.parametrize('budget', [0, 1, 2000, 50000])
def test_depth_zero_is_exact_min_unsat(handle, budget):
    inst, hints, _ = sc.batch()
    seen = set()
    for kind in sc.KINDS:
        want = plain(inst, hints[kind], budget, prob=handle)
        zero = run(inst, hints[kind], 0, budget, prob=handle)
        for k, w in zip(KEYS[:5], want):
            if k == 'model':
                assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(zero[k], w))
            else:
                assert zero[k].dtype == w.dtype and np.array_equal(zero[k], w), k
        assert not zero['depth_used'].any() and np.array_equal(zero['cube_off'], np.arange(len(inst) + 1))
        assert np.array_equal(zero['cube_status'], want[0]) and np.array_equal(zero['cube_improvements'], want[4])
        promised(inst, zero)
        seen |= set(want[0].tolist())
    assert seen == ({1} if budget == 0 else {-1, 1})


def test_budget_per_cube():
    rng = np.random.RandomState(184)
    inst = [cs.threshold_3sat(rng, 40, 184) for _ in range(60)]
    hints = cs.hints_of(rng, inst, 'random')
    depth = np.random.RandomState(8).randint(0, 5, size=len(inst)).astype(np.int8)
    first = np.array([mm.unsat_count(c, h) for (_, c), h in zip(inst, hints)])
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    cubes = 1 << depth.astype(np.int64)
    p = problem(inst)
    seen = set()
    for budget in (2000, 50000):
        got = run(inst, hints, depth, budget, prob=p)
        chk = np.array([sm.check(n, c, h)[4] for (n, c), h in zip(inst, hints)])
        print('budget %d per cube: proved %d of %d, cost sum %d against the hints\' %d, work max %d'
              % (budget, int((got['status'] == 1).sum()), len(inst), int(got['cost'].sum()), int(first.sum()), int(got['work'].max())))
        promised(inst, got, depth)                                                        # a status -1 keeps a model that attains its cost
        per_cube = np.repeat(edges, cubes)
        assert (got['cube_work'] < budget + 3 * per_cube).all()
        assert (np.repeat(chk, cubes)[got['cube_status'] == -1] + got['cube_work'][got['cube_status'] == -1] >= budget).all()
        assert (got['work'] < chk + cubes * (budget + 3 * edges)).all()
        assert np.array_equal(got['work'], chk + np.add.reduceat(got['cube_work'], got['cube_off'][:-1]))
        assert (got['cost'] <= first).all() and (first > 0).all()
        seen |= set(got['status'].tolist())
    assert -1 in seen and (got['cost'] < first).any()


def test_wider_than_a_wave_at_depth_three(monkeypatch):
    "wide(70): n = 151 -- three chunks of lanes, a row of five words, 141 variables forced in one pass"
    (n, clauses), hint = cs.wide(70)
    assert n == 151 and (n + 31) // 32 == 5
    got = run([(n, clauses)], [hint], 3)
    proved([(n, clauses)], got, [2], [3])
    assert got['first'][0] >= 0 and got['improvements'][0] >= 1
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    same_as_sequential(run([(n, clauses)], [hint], 3), [sm.sequential(n, clauses, hint, 0, 3)], 3)


def test_hbm_route_is_searched_at_depth_zero():
    big, hint = cs.past_the_slab()
    rng = np.random.RandomState(4)
    from test_exact_gpu import random_instance
    few = [random_instance(rng, 12) for _ in range(40)]
    fh = cs.hints_of(rng, few, 'random')
    inst, hints = few[:20] + [big] + few[20:], fh[:20] + [hint] + fh[20:]
    p = problem(inst)
    got = run(inst, hints, 3, prob=p)
    want = plain(inst, hints, prob=p)
    assert got['depth_used'][20] == 0 and (np.delete(got['depth_used'], 20) == 3).all()
    assert (got['status'][20], got['cost'][20], got['work'][20], got['improvements'][20]) == (want[0][20], want[1][20], want[3][20], want[4][20])
    assert np.array_equal(got['model'][20], want[2][20]) and got['cost'][20] == cs.brute_min(*big)
    proved(inst, got, want[1], got['depth_used'])
    alone = run([big], [hint], 3)
    assert alone['depth_used'].tolist() == [0] and alone['cost'][0] == got['cost'][20] and alone['work'][0] == got['work'][20]
    assert np.array_equal(alone['model'][0], got['model'][20])


def test_a_prefix_that_ends_early(monkeypatch):
    "n = 3 at depth 8: every leaf lies inside the prefix and belongs to one of the cubes that reach it"
    n, clauses = sc.prefix_only()
    for hint in (None, np.array([1, 0, 1], dtype=np.float32)):
        got = run([(n, clauses)], [hint], 8)
        proved([(n, clauses)], got, [1], [8])
        assert len(got['cube_status']) == 256 and int((got['cube_improvements'] > 0).sum()) <= 8
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    same_as_sequential(run([(n, clauses)], [None], 8), [sm.sequential(n, clauses, None, 0, 8)], 8)


def fields(got, idx=None):
    "the promised fields in a comparable form"
    idx = range(len(got['status'])) if idx is None else idx
    return [(int(got['status'][j]), int(got['cost'][j]), int(got['depth_used'][j]), int(got['cube_off'][j + 1] - got['cube_off'][j])) for j in idx]


def test_the_promised_fields_are_deterministic(handle):
    from pdp import native
    inst, kinds, depth = sc.batch()
    hints = kinds['nan30']
    first = run(inst, hints, depth, prob=handle)
    a = fields(first)
    assert a == fields(run(inst, hints, depth, prob=handle))                              # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    shuffled = run([inst[i] for i in order], [hints[i] for i in order], depth[order])    # a shuffled batch
    assert [a[i] for i in order] == fields(shuffled)
    promised([inst[i] for i in order], shuffled, depth[order])
    for i in list(range(0, len(inst), 31)) + [len(inst) - 1]:                             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            alone = run([inst[i]], [hints[i]], depth[i:i + 1])
            assert [a[i]] == fields(alone)
            promised([inst[i]], alone)
    prev = native.use_build('fast')
    try:
        fast = run(inst, hints, depth)
    finally:
        native.use_build(prev)
    assert a == fields(fast)
    promised(inst, fast, depth)


def test_refusals(tmp_path):
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_min_unsat_split(depth=2)
    p = native.Problem(*args)
    cubes = (torch.empty(p.B + 1, dtype=torch.int64, device=p.device), torch.empty(1 << 10, dtype=torch.int8, device=p.device),
             torch.empty(1 << 10, dtype=torch.int32, device=p.device), torch.empty(1 << 10, dtype=torch.int64, device=p.device),
             torch.empty(1 << 10, dtype=torch.int32, device=p.device))
    assert native.lib().pdp_exact_min_unsat_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK   # no split call yet
    for wrong, at in ((17, 5), (-1, 63)):
        depth = torch.zeros(p.B, dtype=torch.int8, device=p.device)
        depth[at] = wrong
        depth[70] = wrong
        with pytest.raises(native.NativeError, match='depth of instance %d is not in 0 .. 16' % at):
            p.exact_min_unsat_split(depth=depth)
    # a call that must be refused runs with a budget of one read: should the refusal ever fail, its cubes end after one pass each
    with pytest.raises(native.NativeError, match=r'more than 2\^22 cubes in one call \(reached at instance 64\)'):
        p.exact_min_unsat_split(1, depth=16)                                                # 80 * 2^16
    assert native.lib().pdp_exact_min_unsat_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK   # a refused call leaves none
    for wrong in (torch.zeros(p.V + 1, dtype=torch.float32, device=p.device), torch.zeros(p.V - 1, dtype=torch.float32, device=p.device),
                  torch.zeros(p.V, dtype=torch.float64, device=p.device), np.zeros(p.V, dtype=np.float32)):
        with pytest.raises(ValueError):
            p.exact_min_unsat_split(hints=wrong, depth=2)
    for wrong in (1.5, '7', True, torch.zeros(p.B), torch.zeros(p.B - 1, dtype=torch.int8, device=p.device), torch.zeros(p.B, dtype=torch.int8)):
        with pytest.raises(ValueError):
            p.exact_min_unsat_split(depth=wrong)
    st = p.exact_min_unsat_split(depth=3)[0]
    assert (st.cpu().numpy() == 1).all()
    assert native.lib().pdp_exact_min_unsat_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) == native.PDP_OK
    for argv, said in ((['--complete', '--complete-min-unsat-split', '3'], 'give --complete-min-unsat as well'),
                       (['--complete', '--complete-min-unsat', '--complete-min-unsat-split', '17'], 'takes a depth from 0 to 16'),
                       (['--complete', '--complete-min-unsat', '--complete-min-unsat-split', '-2'], 'takes a depth from 0 to 16')):
        r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d'] + argv +
                           ['-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                           cwd=REPO)
        assert r.returncode != 0 and '--complete-min-unsat-split' in r.stderr and said in r.stderr


def test_min_unsat_split_on_segments_and_items_without_a_literal(monkeypatch):
    from pdp import exact
    few, kinds = sc.family()
    more = sc.uniform_3sat(150, 30, 2)
    inst = few[:100] + more
    rng = np.random.RandomState(15)
    hints = [np.array([1, 0, np.nan], dtype=np.float32), None] + kinds['random'][:100] + cs.hints_of(rng, more, 'random') + \
        [np.array([0.2, 0.9, 1, 0], dtype=np.float32)]
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + [exact.raw_item(4, [[]])]
    base = exact.min_unsat(raw, hints=hints)
    assert (base[0] == 1).all() and base[1][0] == 0 and base[1][1] == 2 and base[1][-1] == 1
    monkeypatch.setattr(exact, 'AUTO_MIN_STAGE1_BUDGET', 300)                             # so that the second stage has work to do
    for split in (4, 'auto'):
        for max_edges in (exact.MAX_EDGES, 400):
            got = exact.min_unsat(raw, hints=hints, split=split, max_edges=max_edges, depths=True)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
            assert (got[0].dtype, got[1].dtype, got[3].dtype, got[4].dtype) == (np.int8, np.int32, np.int64, np.int8)
            for it, (n, c), m, co in zip(raw[2:-1], inst, got[2][2:-1], got[1][2:-1]):
                assert m.dtype == np.float32 and len(m) == n and mm.unsat_count(c, m) == co
            assert [m.tolist() for m in (got[2][0], got[2][1], got[2][-1])] == [[1, 0, 0], [0, 0], [0, 1, 1, 0]]
            assert got[3][0] == got[3][1] == got[3][-1] == 0
            if split == 4:
                assert (got[4] == 4).all() or max_edges == 400
                assert (got[4][2:-1] == 4).all()
            else:
                assert (got[4] > 0).sum() >= 5 and (got[4] == 0).sum() >= 5              # some rows end in the first stage, some do not
                assert (got[3][got[4] > 0] > 300).all()                                    # work is the sum of both stages
    assert len(exact.min_unsat(raw[:5], hints=hints[:5], split=2)) == 4


def test_cli_complete_min_unsat_split(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    for i in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 138)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete', '--complete-min-unsat']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-min-unsat-split', '3'], 1, str(tmp_path / 'deep.jsonl'), 0)
    auto, _ = _run(argv + ['--complete-min-unsat-split', '-1'], 1, str(tmp_path / 'auto.jsonl'), 0)
    assert len(base) == len(deep) == len(auto) == 40
    split = 0
    for b, d in zip(base, deep):
        r, rb = json.loads(d), json.loads(b)
        if rb['complete'] == 1:
            assert d == b                                                                # byte-identical to the run without the flag
            continue
        assert list(r)[-2:] == ['min_unsat_work', 'min_unsat_split_depth'] and list(r)[:-1] == list(rb) and r['min_unsat_split_depth'] == 3
        moved = ('min_unsat_solution', 'min_unsat_work', 'min_unsat_split_depth')
        assert {k: v for k, v in r.items() if k not in moved} == {k: v for k, v in rb.items() if k not in moved}
        assert rb['min_unsat_proved'] == 1 and r['min_unsat'] >= 1 and r['min_unsat_work'] > 0
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        assert len(r['min_unsat_solution']) == n and mm.unsat_count(clauses, r['min_unsat_solution']) == r['min_unsat']
        split += 1
    assert split >= 5
    assert auto == base                                                                   # every row is proved by the plain first stage
