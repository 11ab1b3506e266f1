"""The split counting search on the GPU (pdp_exact_count_split, Problem.exact_count_split, exact.count_models(split=), satyr.py --complete
--complete-count --complete-count-split): equal to its Python statement (tests/exact_count_split_model.py) bit for bit in status, count,
true_count, work, leaves, depth_used and every cube record; depth 0 equal to exact_count; count, true_count and leaves equal to exact_count
at every depth where the count is exact; the budget per cube; determinism of every output and record over call, batch, grid and build;
the HBM route and instances that are too large; refusals; the host entry points; the command line."""
import ctypes
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_count_model as cm
import exact_count_split_model as sm
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
KEYS = ('status', 'count', 'true_count', 'work', 'leaves', 'depth_used', 'cube_off', 'cube_status', 'cube_count', 'cube_work', 'cube_leaves')
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
    return [(max([n] + [abs(l) for cl in c for l in cl]), c) for n, c in inst]


def run(inst, depth, budget=0, prob=None):
    "Problem.exact_count_split(stats=True) as a dict of numpy arrays, true_count cut per instance"
    p = problem(inst) if prob is None else prob
    d = depth if isinstance(depth, int) else torch.from_numpy(np.asarray(depth, dtype=np.int8)).cuda()
    got = dict(zip(KEYS, [t.cpu().numpy() for t in p.exact_count_split(budget, depth=d, stats=True)]))
    assert [got[k].dtype for k in KEYS] == [np.int8, np.float64, np.float64, np.int64, np.int64, np.int8, np.int64, np.int8, np.float64,
                                            np.int64, np.int64]
    assert got['cube_off'][0] == 0 and np.array_equal(np.diff(got['cube_off']), 1 << got['depth_used'].astype(np.int64))
    assert got['cube_status'].shape == got['cube_count'].shape == got['cube_work'].shape == got['cube_leaves'].shape == (got['cube_off'][-1],)
    got['true_count'] = np.split(got['true_count'], np.cumsum([n for n, _ in inst])[:-1])
    return got


def reference(inst, depth, budget=0):
    depth = [depth] * len(inst) if isinstance(depth, int) else depth
    return [sm.search(n, c, budget, int(d)) for (n, c), d in zip(inst, depth)]


def same_as_model(got, want, depth):
    "every output and every cube record against tests/exact_count_split_model.py, bit for bit"
    depth = [depth] * len(want) if isinstance(depth, int) else depth
    for j, (st, count, tc, work, leaves, cubes) in enumerate(want):
        assert (got['status'][j], got['count'][j], got['work'][j], got['leaves'][j], got['depth_used'][j]) == (st, count, work, leaves, depth[j]), j
        assert np.array_equal(got['true_count'][j], tc), j
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        rec = list(zip(got['cube_status'][a:z].tolist(), got['cube_count'][a:z].tolist(), got['cube_work'][a:z].tolist(),
                       got['cube_leaves'][a:z].tolist()))
        assert rec == [tuple(c) for c in cubes], j


def everything(got, order=None):
    "every output and record per instance in a comparable form"
    idx = range(len(got['status'])) if order is None else order
    out = []
    for j in idx:
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        out.append((int(got['status'][j]), got['count'][j].tobytes(), got['true_count'][j].tobytes(), int(got['work'][j]), int(got['leaves'][j]),
                    int(got['depth_used'][j]), got['cube_status'][a:z].tobytes(), got['cube_count'][a:z].tobytes(),
                    got['cube_work'][a:z].tobytes(), got['cube_leaves'][a:z].tobytes()))
    return out


@pytest.fixture(scope='module')
def batch():
    """about 430 instances in one problem: the host family (n <= 12), the two fans at depth 2, uniform 3-SAT of n = 20 / 30 at clause ratios
    3.5, 4.0 and 4.5; depths mixed over 0..6; the model's answers, computed once"""
    few = cs.family()
    inst = widen(few + [cs.fan(k) for k in cs.FAN_K] + cs.uniform_3sat(20, 20, (3.5, 4.0, 4.5), 3) + cs.uniform_3sat(30, 30, (3.5, 4.0, 4.5), 3))
    depth = np.random.RandomState(7).randint(0, 7, size=len(inst)).astype(np.int8)
    depth[len(few):len(few) + len(cs.FAN_K)] = 2
    return inst, depth, reference(inst, depth), problem(inst)


def test_equal_to_the_python_model_exactly(batch):
    inst, depth, want, p = batch
    assert len(inst) >= 425 and set(depth.tolist()) == set(range(7))
    got = run(inst, depth, prob=p)
    inside = sum(1 for w in want if len(w[5]) > 1 and any(c[3] == 0 and c[2] > 0 for c in w[5]))
    print('count split: %d instances, %d cubes, %d with models, %d cubes without a model, leaves max %d'
          % (len(inst), len(got['cube_status']), int((got['count'] > 0).sum()), int((got['cube_count'] == 0).sum()), int(got['leaves'].max())))
    same_as_model(got, want, depth)
    assert (got['status'] == 1).all() and int((got['count'] > 0).sum()) > 250 and int((got['count'] == 0).sum()) > 50 and inside > 100
    few = len(cs.family())
    for j, (bc, bt) in enumerate(cs.family_brute()):                                      # brute force for the n <= 12 part
        assert got['count'][j] == bc and got['true_count'][j].tolist() == bt.tolist()
    for j, k in enumerate(cs.FAN_K):                                                      # 150 forced variables on one level: three chunks of lanes
        assert got['count'][few + j] >= 2.0 ** k and got['leaves'][few + j] == 2 and got['depth_used'][few + j] == 2


def test_depth_zero_is_exact_count(batch):
    inst, _, _, p = batch
    plain = [t.cpu().numpy() for t in p.exact_count(stats=True)]
    zero = run(inst, 0, prob=p)
    for k, want in zip(KEYS[:5], plain):
        got = np.concatenate(zero[k]) if k == 'true_count' else zero[k]
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    assert not zero['depth_used'].any() and np.array_equal(zero['cube_off'], np.arange(len(inst) + 1))
    assert np.array_equal(zero['cube_status'], plain[0]) and np.array_equal(zero['cube_count'], plain[1])
    assert np.array_equal(zero['cube_work'], plain[3]) and np.array_equal(zero['cube_leaves'], plain[4])


def test_equal_to_exact_count_at_n_50():
    from pdp import exact
    inst = cs.uniform_3sat(57, 50, (4.0, 4.26, 4.5, 5.0), 8)
    model = cm.solve(inst, 1 << 22)
    assert len(inst) == 32 and (model[0] == 1).all() and (model[3] < 1 << 22).all()      # all finish under 2^22 reads
    p = problem(inst)
    st, count, tc, work, leaves = [t.cpu().numpy() for t in p.exact_count(stats=True)]
    cs.same((st, count, np.split(tc, np.cumsum([n for n, _ in inst])[:-1]), work, leaves), model)
    sure = exact.count_is_exact(st, count)
    assert sure.all() and (count > 0).sum() >= 8
    for depth in (6, 10):
        got = run(inst, depth, prob=p)
        print('n=50 depth %d: work ratio to the plain count %.2f, cubes without a model %d of %d'
              % (depth, got['work'].sum() / work.sum(), int((got['cube_count'] == 0).sum()), len(got['cube_count'])))
        assert (got['depth_used'] == depth).all()
        assert np.array_equal(got['status'][sure], st[sure]) and np.array_equal(got['count'][sure], count[sure])
        assert np.array_equal(got['leaves'][sure], leaves[sure]) and np.array_equal(np.concatenate(got['true_count']), tc)
        assert (got['work'] >= work).all()
        assert p.exact_last_grid() > 32                     # more waves at work than instances


def test_budget_per_cube():
    inst = widen(cs.family()[::5] + cs.uniform_3sat(184, 30, (3.5, 4.0, 4.6), 3))
    depth = np.random.RandomState(8).randint(0, 5, size=len(inst)).astype(np.int8)
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    full = run(inst, depth, prob=p)
    seen = set()
    for budget in (2000, 50000):
        got = run(inst, depth, budget, prob=p)
        same_as_model(got, reference(inst, depth, budget), depth)
        per_cube = np.repeat(edges, 1 << depth.astype(np.int64))
        assert (got['cube_work'] < budget + 3 * per_cube).all() and (got['cube_work'][got['cube_status'] == -1] >= budget).all()
        assert (got['work'] < (1 << depth.astype(np.int64)) * (budget + 3 * edges)).all()
        assert (got['count'] <= full['count']).all() and (got['leaves'] <= full['leaves']).all()
        for j in range(len(inst)):
            a, z = got['cube_off'][j], got['cube_off'][j + 1]
            assert got['status'][j] == (-1 if (got['cube_status'][a:z] == -1).any() else 1)
        seen |= set(got['status'].tolist())
    assert seen == {-1, 1} and ((got['status'] == -1) & (got['count'] > 0)).any()


def test_deterministic_in_every_output_and_record(batch, monkeypatch):
    from pdp import native
    inst, depth, _, p = batch
    a = everything(run(inst, depth, prob=p))
    assert a == everything(run(inst, depth, prob=p))                                      # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    assert [a[i] for i in order] == everything(run([inst[i] for i in order], depth[order]))      # a shuffled batch
    for i in list(range(0, len(inst), 61)) + [len(inst) - 1]:                             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            assert [a[i]] == everything(run([inst[i]], depth[i:i + 1]))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every cube, one after the other
    one = run(inst, depth, prob=p)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    assert a == everything(one)
    run(inst, depth, prob=p)
    assert p.exact_last_grid() > 1
    prev = native.use_build('fast')
    try:
        fast = run(inst, depth)
    finally:
        native.use_build(prev)
    assert a == everything(fast)


def test_hbm_route_is_counted_at_depth_zero():
    big = cs.past_the_slab()
    few = cs.family()[:40]
    inst = widen(few[:20] + [big] + few[20:])
    p = problem(inst)
    got = run(inst, 3, prob=p)
    want = cs.slab_result()
    assert got['depth_used'][20] == 0 and (np.delete(got['depth_used'], 20) == 3).all()
    assert (got['status'][20], got['count'][20], got['work'][20], got['leaves'][20]) == (want[0], want[1], want[3], want[4])
    assert np.array_equal(got['true_count'][20], want[2])
    rest = [i for i in range(len(inst)) if i != 20]
    brute = cs.family_brute()[:40]
    assert [got['count'][i] for i in rest] == [b[0] for b in brute]
    assert all(got['true_count'][i].tolist() == b[1].tolist() for i, b in zip(rest, brute))
    alone = run([inst[20]], 3)
    assert alone['depth_used'].tolist() == [0] and everything(alone) == everything(got, [20])


def test_too_many_variables_in_a_batch():
    few = widen(cs.family()[:6])
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    edge = (1023, [[1, 2], [-1, 1023]])
    inst = few[:3] + [wide] + few[3:] + [edge]
    depth = [2, 0, 5, 4, 1, 3, 6, 2]
    got = run(inst, depth)
    assert got['status'].tolist() == [1, 1, 1, -2, 1, 1, 1, 1] and got['depth_used'].tolist() == [2, 0, 5, 0, 1, 3, 6, 2]
    assert (got['count'][3], got['work'][3], got['leaves'][3]) == (0.0, 0, 0) and got['true_count'][3].shape == (1024,)
    assert not got['true_count'][3].any()
    same_as_model(got, reference(inst, depth), got['depth_used'].tolist())
    assert got['count'][7] == 2.0 ** 1022 and np.isfinite(got['true_count'][7]).all()
    alone = run([wide], 7)
    assert everything(alone) == everything(got, [3])


def test_refusals(tmp_path):
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_count_split(depth=2)
    p = native.Problem(*args)
    cubes = (torch.empty(p.B + 1, dtype=torch.int64, device=p.device), torch.empty(1 << 10, dtype=torch.int8, device=p.device),
             torch.empty(1 << 10, dtype=torch.float64, device=p.device), torch.empty(1 << 10, dtype=torch.int64, device=p.device),
             torch.empty(1 << 10, dtype=torch.int64, device=p.device))
    assert native.lib().pdp_exact_count_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK       # no split call yet
    for wrong, at in ((17, 5), (-1, 63)):
        depth = torch.zeros(p.B, dtype=torch.int8, device=p.device)
        depth[at] = wrong
        depth[70] = wrong
        with pytest.raises(native.NativeError, match='depth of instance %d is not in 0 .. 16' % at):
            p.exact_count_split(depth=depth)
    # every call that must be refused runs with a budget of one read: should a refusal ever fail, its cubes end after one pass each
    with pytest.raises(native.NativeError, match=r'more than 2\^22 cubes in one call \(reached at instance 64\)'):
        p.exact_count_split(1, depth=16)                                                    # 80 * 2^16
    # the rows: cubes x n_max x 8 bytes.  At n = 8 the cube cap comes first; 12 instances of 600 variables (most of them in no clause:
    # raw_item keeps them) pass 2^31 bytes at the seventh: 7 * 2^16 * 600 * 8 > 2^31 >= 6 * 2^16 * 600 * 8
    rng = np.random.RandomState(2)
    q = problem([(600, [[int(v) * int(s) for v, s in zip(rng.choice(600, size=3, replace=False) + 1, rng.choice([-1, 1], size=3))]
                        for _ in range(60)]) for _ in range(12)])
    assert q.V == 12 * 600
    with pytest.raises(native.NativeError, match=r'per-cube rows \(cubes x 600 variables x 8 bytes\) pass 2\^31 bytes at instance 6'):
        q.exact_count_split(1, depth=16)
    assert native.lib().pdp_exact_count_split_cubes(q._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK       # a refused call leaves none
    ok = torch.zeros(q.B, dtype=torch.int8, device=q.device)
    ok[:6] = 12
    st, count = q.exact_count_split(1, depth=ok)[:2]                                        # 6 * 2^12 + 6 cubes of 600 variables: allowed
    assert (st.cpu().numpy() == -1).all() and not count.cpu().numpy().any()                 # one read each: nothing is counted
    for wrong in (1.5, '7', True, torch.zeros(p.B), torch.zeros(p.B - 1, dtype=torch.int8, device=p.device), torch.zeros(p.B, dtype=torch.int8)):
        with pytest.raises(ValueError):
            p.exact_count_split(depth=wrong)
    for wrong in (1.5, '7', None, True):
        with pytest.raises(ValueError):
            p.exact_count_split(budget=wrong)
    status = torch.empty(p.B, dtype=torch.int8, device=p.device)
    assert native.lib().pdp_exact_count_split(p._h, None, ctypes.c_int64(0), native.ptr(status), None, None, None, None, None, None) != native.PDP_OK
    st = p.exact_count_split(depth=3)[0]
    assert (st.cpu().numpy() == 1).all()
    for argv, said in ((['--complete', '--complete-count-split', '3'], 'give --complete-count as well'),
                       (['--complete', '--complete-count', '--complete-count-split', '17'], 'takes a depth from 0 to 16'),
                       (['--complete', '--complete-count', '--complete-count-split', '-2'], 'takes a depth from 0 to 16')):
        r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d'] + argv +
                           ['-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                           cwd=REPO)
        assert r.returncode != 0 and '--complete-count-split' in r.stderr and said in r.stderr


def test_count_models_split_on_segments_and_items_without_a_literal(monkeypatch):
    from pdp import exact
    inst = cs.family()[:120] + cs.uniform_3sat(150, 30, (3.5, 4.26, 5.0), 3)
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + \
        [exact.raw_item(4, [[]]), exact.raw_item(1024, []), exact.raw_item(1024, [[1, 2], [-1, 1024]])]
    base = exact.count_models(raw)
    assert set(base[0].tolist()) == {-2, 1} and exact.count_is_exact(base[0], base[1])[:-2].all()
    monkeypatch.setattr(exact, 'AUTO_COUNT_STAGE1_BUDGET', 300)                           # so that the second stage has work to do
    for split in (4, 'auto'):
        for max_edges in (exact.MAX_EDGES, 400):
            got = exact.count_models(raw, split=split, max_edges=max_edges, depths=True)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
            assert (got[0].dtype, got[1].dtype, got[3].dtype, got[4].dtype) == (np.int8, np.float64, np.int64, np.int8)
            for a, b in zip(got[2], base[2]):
                assert (a is None) == (b is None) and (a is None or (a.dtype == np.float64 and np.array_equal(a, b)))
            assert (got[3] >= base[3]).all() and got[3][0] == got[3][1] == got[3][-3] == got[3][-2] == got[3][-1] == 0
            assert got[4][-2] == got[4][-1] == 0 and got[4].max() > 0                  # more than 1023 variables: one cube
            if split == 4:
                assert (got[4][:-2] == 4).all()
            else:
                assert (got[4] > 0).sum() >= 5 and (got[4] == 0).sum() >= 5              # some rows end in the first stage, some do not
                assert (got[3][got[4] > 0] > base[3][got[4] > 0]).all()                    # work is the sum of both stages
    assert len(exact.count_models(raw[:5], split=2)) == 4


def test_cli_complete_count_split(tmp_path):
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
    deep, _ = _run(argv + ['--complete-count-split', '3'], 1, str(tmp_path / 'deep.jsonl'), 0)
    auto, _ = _run(argv + ['--complete-count-split', '-1'], 1, str(tmp_path / 'auto.jsonl'), 0)
    assert len(base) == len(deep) == len(auto) == 40
    split = 0
    for b, d in zip(base, deep):
        r, rb = json.loads(d), json.loads(b)
        if 'count_split_depth' not in r:
            assert d == b and rb['complete'] != 1                                        # byte-identical to the run without the flag
            continue
        assert r['count_split_depth'] == 3 and list(r)[-2:] == ['count_work', 'count_split_depth']
        assert list(r)[:-1] == list(rb)
        assert {k: v for k, v in r.items() if k not in ('count_work', 'count_split_depth')} == {k: v for k, v in rb.items() if k != 'count_work'}
        assert r['count_work'] >= rb['count_work'] and rb['model_count_proved'] == 1
        split += 1
    assert split >= 5
    assert auto == base                                                                   # every row is counted by the plain first stage
