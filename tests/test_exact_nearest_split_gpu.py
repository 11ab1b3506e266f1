"""The split nearest-model search on the GPU (pdp_exact_nearest_split, Problem.exact_nearest_split, exact.nearest_model(split=, start=),
satyr.py --complete --complete-nearest --complete-nearest-split).  With one wave (PDP_EXACT_GRID=1, in a process of its own) every output
and cube record equals the Python statement's sequential() (tests/exact_nearest_split_model.py) bit for bit.  With the full grid only what
is promised is compared: status and cost (against the plain statement, exact_nearest on the same handle and pdp_cnf_eval), a model at that
distance, the cube that holds it, depth_used, start_cost.  Depth 0 equal to exact_nearest in all five outputs under every budget; the budget
per cube; the constructed cases (the pinned flip, a 64-bit cost, the hint fill past 64 variables, instances wider than a wave, the HBM
route, a prefix that ends early, a penalty out of range); determinism of the promised fields; reuse of one handle; refusals; the host entry
point; the command line.  Which minimiser comes back, first, work, improvements and the records depend on timing above one wave and are
not compared."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_nearest_cases as nc
import exact_nearest_model as nm
import exact_nearest_split_cases as sc
import exact_nearest_split_model as sm
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
KEYS = ('status', 'cost', 'model', 'work', 'improvements', 'first', 'depth_used', 'start_cost', 'cube_off', 'cube_status', 'cube_cost',
        'cube_work', 'cube_improvements')
DTYPES = [np.int8, np.int64, np.float32, np.int64, np.int32, np.int32, np.int8, np.int64, np.int64, np.int8, np.int64, np.int64, np.int32]
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


def flat(p, inst, per, dtype, fill):
    "None: a NULL pointer; an instance without an entry gets ``fill``"
    if per is None:
        return None
    rows = [np.full(n, fill, dtype=dtype) if h is None else np.asarray(h, dtype=dtype) for (n, _), h in zip(inst, per)]
    return torch.from_numpy(np.concatenate(rows)).to(p.device)


def run(inst, hints, pens, begin, depth, budget=0, prob=None):
    "Problem.exact_nearest_split(stats=True) as a dict of numpy arrays, the model cut per instance"
    p = problem(inst) if prob is None else prob
    d = depth if isinstance(depth, int) else torch.from_numpy(np.asarray(depth, dtype=np.int8)).cuda()
    out = p.exact_nearest_split(flat(p, inst, hints, np.float32, 0.0), flat(p, inst, pens, np.int32, 1), flat(p, inst, begin, np.float32, 0.0),
                                depth=d, budget=budget, stats=True)
    got = dict(zip(KEYS, [t.cpu().numpy() for t in out]))
    assert [got[k].dtype for k in KEYS] == DTYPES
    assert got['cube_off'][0] == 0 and np.array_equal(np.diff(got['cube_off']), 1 << got['depth_used'].astype(np.int64))
    assert got['cube_status'].shape == got['cube_cost'].shape == got['cube_work'].shape == got['cube_improvements'].shape == (got['cube_off'][-1],)
    got['model'] = np.split(got['model'], np.cumsum([n for n, _ in inst])[:-1])
    return got


def plain(inst, hints, pens, budget=0, prob=None):
    "Problem.exact_nearest(stats=True) in the layout of exact_nearest_model.solve"
    p = problem(inst) if prob is None else prob
    out = p.exact_nearest(flat(p, inst, hints, np.float32, 0.0), flat(p, inst, pens, np.int32, 1), budget, stats=True)
    st, cost, model, work, imp = [t.cpu().numpy() for t in out]
    return st, cost, np.split(model, np.cumsum([n for n, _ in inst])[:-1]), work, imp


def same_as_sequential(got, want, depth):
    "every output and every cube record against the statement's sequential(), bit for bit"
    depth = [depth] * len(want) if isinstance(depth, int) else depth
    for j, (st, cost, model, work, imp, first, start_cost, cubes) in enumerate(want):
        assert (got['status'][j], got['cost'][j], got['work'][j], got['improvements'][j], got['first'][j], got['depth_used'][j],
                got['start_cost'][j]) == (st, cost, work, imp, first, depth[j], start_cost), j
        assert np.array_equal(got['model'][j], model), j
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        rec = list(zip(got['cube_status'][a:z].tolist(), got['cube_work'][a:z].tolist(), got['cube_cost'][a:z].tolist(),
                       got['cube_improvements'][a:z].tolist()))
        assert rec == [tuple(c) for c in cubes], j


def promised(inst, hints, pens, got, depth=None):
    "what holds at any grid and any budget: the model attains the cost, the cube named by first holds it, the records add up"
    for j, (n, c) in enumerate(inst):
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        f, cost = got['first'][j], got['cost'][j]
        if got['status'][j] == -3:
            assert (cost, got['work'][j], got['improvements'][j], f, got['start_cost'][j]) == (0, 0, 0, -1, -1) and not got['model'][j].any()
            continue
        assert got['status'][j] == (-1 if (got['cube_status'][a:z] != 1).any() else (1 if cost >= 0 else 0)), j
        assert got['improvements'][j] == got['cube_improvements'][a:z].sum(), j
        held = got['cube_cost'][a:z]
        if cost < 0:
            assert cost == -1 and f == -1 and not got['model'][j].any() and (held == sm.NO_COST).all(), j
            continue
        bits = nm.threshold(n, None if hints is None else hints[j])
        pen = nm.penalty_list(n, None if pens is None else pens[j])
        assert nc.satisfies(c, got['model'][j]) and nm.distance(bits, pen, got['model'][j]) == cost, j
        assert -1 <= f < z - a and (got['cube_cost'][a + f] == cost if f >= 0 else cost in (0, got['start_cost'][j])), j
        assert ((held == sm.NO_COST) | (held >= cost)).all(), j
        assert got['start_cost'][j] < 0 or cost <= got['start_cost'][j], j
    assert set(np.unique(got['cube_status']).tolist()) <= {-1, 1}
    if depth is not None:
        assert np.array_equal(got['depth_used'], np.asarray(depth, dtype=np.int8))


def proved(inst, hints, pens, got, want, depth):
    "with a budget that no cube exhausts: the plain search's status and cost, on top of promised()"
    promised(inst, hints, pens, got, depth)
    assert (got['cube_status'] == 1).all()
    np.testing.assert_array_equal(got['status'], want[0])
    np.testing.assert_array_equal(got['cost'], want[1])


@pytest.fixture(scope='module')
def handle():
    return problem(sc.batch()[0])


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import exact_nearest_split_cases as sc
import test_exact_nearest_split_gpu as t
inst, _, _, depth = sc.batch()
p = t.problem(inst)
out = {}
for variant in sc.VARIANTS:
    hints, pens, begin = sc.dressed(variant)
    r = t.run(inst, hints, pens, begin, depth, prob=p)
    r['model'] = np.concatenate(r['model'])
    out.update({variant + '_' + k: v for k, v in r.items()})
    out[variant + '_grid'] = p.exact_last_grid()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope='module')
def one_wave(tmp_path_factory):
    "the three variants of the batch with PDP_EXACT_GRID=1: one wave takes every cube, one after the other, in a process of its own"
    out = str(tmp_path_factory.mktemp('one_wave') / 'one.npz')
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    r = subprocess.run([sys.executable, '-c', CHILD % (os.path.join(REPO, 'tests'), os.path.join(REPO, 'pdp-solver_amd')), out],
                       env=dict(os.environ, PDP_EXACT_GRID='1'), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=STEP_LIMIT, cwd=REPO)
    faulthandler.cancel_dump_traceback_later()
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize('variant', sc.VARIANTS)
def test_one_wave_equals_the_python_model_exactly(one_wave, variant):
    inst, _, _, depth = sc.batch()
    hints, pens, begin = sc.dressed(variant)
    got = {k: one_wave[variant + '_' + k] for k in KEYS}
    assert int(one_wave[variant + '_grid']) == 1
    got['model'] = np.split(got['model'], np.cumsum([n for n, _ in inst])[:-1])
    want = sc.batch_sequential(variant)
    print('nearest split, %s: %d instances, %d cubes, %d improved, %d cubes with an improvement, %d start models accepted, work %d'
          % (variant, len(inst), len(got['cube_status']), int((got['improvements'] > 0).sum()), int((got['cube_improvements'] > 0).sum()),
             int((got['start_cost'] >= 0).sum()), int(got['work'].sum())))
    same_as_sequential(got, want, depth.tolist())
    proved(inst, hints, pens, got, sc.batch_plain(variant), depth)
    assert int((got['improvements'] > 0).sum()) > 30 and int((got['first'] == -1).sum()) > 5
    assert (int((got['start_cost'] >= 0).sum()) > 50) == (variant == 'start')


@pytest.mark.parametrize('variant', sc.VARIANTS)
def test_full_grid_keeps_what_is_promised(handle, variant):
    inst, _, _, depth = sc.batch()
    hints, pens, begin = sc.dressed(variant)
    got = run(inst, hints, pens, begin, depth, prob=handle)
    assert handle.exact_last_grid() > 1
    proved(inst, hints, pens, got, sc.batch_plain(variant), depth)
    st, cost = plain(inst, hints, pens, prob=handle)[:2]                                  # exact_nearest on the same handle
    np.testing.assert_array_equal(got['status'], st)
    np.testing.assert_array_equal(got['cost'], cost)
    if begin is not None:
        want = [nm.distance(nm.threshold(n, h), nm.penalty_list(n, q), s) if nc.satisfies(c, s) else -1
                for (n, c), h, q, s in zip(inst, hints, pens, begin)]
        np.testing.assert_array_equal(got['start_cost'], want)
    else:
        assert (got['start_cost'] == -1).all()
    # the library's own evaluator: the instances it can take (no empty clause, at least one clause) and that have a model
    keep = [i for i, (n, c) in enumerate(inst) if len(c) > 0 and all(len(x) > 0 for x in c) and st[i] == 1]
    sub = [inst[i] for i in keep]
    p = problem(sub)
    pick = lambda per: None if per is None else [per[i] for i in keep]
    r = run(sub, pick(hints), pick(pens), pick(begin), depth[keep], prob=p)
    _, unsat = p.cnf_eval(torch.from_numpy(np.concatenate(r['model'])).cuda())
    assert not unsat.cpu().numpy().any()
    np.testing.assert_array_equal(r['cost'], cost[keep])


@pytest.mark.parametrize('budget', [0, 1, 2000, 50000])
def test_depth_zero_is_exact_nearest(handle, budget):
    inst, _, _, _ = sc.batch()
    seen = set()
    for variant in ('mixed', 'unit'):
        hints, pens, _ = sc.dressed(variant)
        want = plain(inst, hints, pens, budget, prob=handle)
        zero = run(inst, hints, pens, None, 0, budget, prob=handle)
        for k, w in zip(KEYS[:5], want):
            if k == 'model':
                assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(zero[k], w))
            else:
                assert zero[k].dtype == w.dtype and np.array_equal(zero[k], w), k
        assert not zero['depth_used'].any() and np.array_equal(zero['cube_off'], np.arange(len(inst) + 1))
        assert np.array_equal(zero['cube_improvements'], want[4]) and (zero['start_cost'] == -1).all()
        promised(inst, hints, pens, zero)
        seen |= set(want[0].tolist())
    assert seen == {0, 1} if budget == 0 else {-1, 1} <= seen


def test_budget_per_cube():
    "the n = 50 instances at depth 4, with a model as the start model"
    inst, hints, pens = [[x for (n, _), x in zip(nc.uniform()[0], per) if n == 50] for per in nc.uniform()]
    assert len(inst) == 6
    rng = np.random.RandomState(50)
    begin = [nc.any_model(n, c) for n, c in inst]
    begin = [rng.randint(0, 2, size=n).astype(np.float32) if m is None else m for (n, _), m in zip(inst, begin)]
    edges = nc.edges(inst)
    cubes = np.full(len(inst), 16, dtype=np.int64)
    p = problem(inst)
    seen = set()
    for budget in (2000, 50000):
        got = run(inst, hints, pens, begin, 4, budget, prob=p)
        chk = np.array([sm.check(n, c, h, q, s)[4] for (n, c), h, q, s in zip(inst, hints, pens, begin)])
        print('budget %d per cube: proved %d of %d, cost %s against the start models\' %s, work max %d'
              % (budget, int((got['status'] == 1).sum()), len(inst), got['cost'].tolist(), got['start_cost'].tolist(), int(got['work'].max())))
        promised(inst, hints, pens, got, [4] * len(inst))                                  # a status -1 keeps a model that attains its cost
        per_cube = np.repeat(edges, cubes)
        assert (got['cube_work'] < budget + 3 * per_cube).all()
        assert (np.repeat(chk, cubes)[got['cube_status'] == -1] + got['cube_work'][got['cube_status'] == -1] >= budget).all()
        assert (got['work'] < chk + cubes * (budget + 3 * edges)).all()
        assert np.array_equal(got['work'], chk + np.add.reduceat(got['cube_work'], got['cube_off'][:-1]))
        given = got['start_cost'] >= 0
        assert given.sum() >= 3 and (got['cost'][given] <= got['start_cost'][given]).all() and (got['cost'][given] >= 0).all()
        seen |= set(got['status'].tolist())
    assert -1 in seen


def test_constructed_cases(monkeypatch):
    """the pinned flip (fan_case, depth 2), a 64-bit cost through the shared word and the finish (units_case, 4 100 * 2^20 > 2^32: past
    the slab, so its one cube runs at depth 0), 1 500 units at depth 3 (1 500 * 2^20, above 2^30, from a row of 47 words), the row's fill
    with hint values past 64 variables (fill_case, depth 3).  A cost above 2^32 needs more than 4 096 variables, and the slab holds
    far fewer: no instance above depth 0 can reach one, so the word's upper half is exercised through the depth-0 cube alone; the
    shared-word code is the same at every depth."""
    units = (1500, [[i + 1] for i in range(1500)]), np.zeros(1500, dtype=np.float32), np.full(1500, nc.CAP, dtype=np.int32)
    cases = [nc.fan_case(150), nc.units_case(4100), nc.fill_case(100), units]
    inst, hints, pens = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    depth, used = [2, 3, 3, 3], [2, 0, 3, 3]
    want = nm.solve(inst, hints, pens)
    assert want[0].tolist() == [1, 1, 1, 1] and want[1].tolist() == [150, 4100 << 20, 5, 1500 << 20]
    got = run(inst, hints, pens, None, depth)
    proved(inst, hints, pens, got, want, used)
    assert got['model'][2][12:].all() and len(got['model'][2]) == 112 and got['model'][3].all()
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    one = run(inst, hints, pens, None, depth)
    same_as_sequential(one, sm.solve(inst, hints, pens, None, depths=used), used)
    a = one['cube_off'][0]
    first_pass = int(nc.edges(inst[:1])[0])
    assert one['cube_work'][a + 2] == one['cube_work'][a + 3] == 3 * first_pass           # no pass behind the pin


def test_wide_instances_at_depth_three(monkeypatch):
    "trails past 128, passes of 100 units, levels of more than 64 entries undone, under a budget per cube"
    inst, hints, pens = nc.wide_batch()
    budget = 30000                                                                        # per cube: the large ones end as upper bounds
    got = run(inst, hints, pens, None, 3, budget)
    used = got['depth_used'].tolist()
    assert set(used) <= {0, 3} and used.count(3) >= 20                                    # 0: an instance past the slab
    promised(inst, hints, pens, got, used)
    want, _ = nc.wide_results()
    done = (got['status'] != -1) & (want[0] != -1)
    assert done.sum() >= 10 and np.array_equal(got['status'][done], want[0][done]) and np.array_equal(got['cost'][done], want[1][done])
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    one = run(inst, hints, pens, None, 3, budget)
    same_as_sequential(one, sm.solve(inst, hints, pens, None, budget, depths=used), used)
    assert (one['status'] == -1).sum() >= 5 and (one['improvements'] > 0).sum() >= 5


def test_hbm_route_is_searched_at_depth_zero():
    big, hint, pen = nc.slab_case()
    few, fh, fp = [x[:40] for x in nc.small()]
    inst, hints, pens = few[:20] + [big] + few[20:], fh[:20] + [hint] + fh[20:], fp[:20] + [pen] + fp[20:]
    p = problem(inst)
    got = run(inst, hints, pens, None, 3, prob=p)
    want = plain(inst, hints, pens, prob=p)
    ref = nc.slab_result()
    assert got['depth_used'][20] == 0 and (np.delete(got['depth_used'], 20) == 3).all()
    assert (got['status'][20], got['cost'][20], got['work'][20], got['improvements'][20]) == (want[0][20], want[1][20], want[3][20], want[4][20])
    assert (want[0][20], want[1][20], want[3][20], want[4][20]) == (ref[0], ref[1], ref[3], ref[4])
    assert np.array_equal(got['model'][20], want[2][20]) and np.array_equal(got['model'][20], ref[2])
    proved(inst, hints, pens, got, want, got['depth_used'])
    alone = run([big], [hint], [pen], None, 3)
    assert alone['depth_used'].tolist() == [0] and alone['cost'][0] == got['cost'][20] and alone['work'][0] == got['work'][20]
    assert np.array_equal(alone['model'][0], got['model'][20])


def test_a_prefix_that_ends_early(monkeypatch):
    "n = 3 at depth 8: every leaf lies inside the prefix and belongs to one of the cubes that reach it"
    n, clauses = sc.prefix_only()
    for hint in (None, np.array([1, 0, 1], dtype=np.float32)):
        want = nm.solve([(n, clauses)], [hint])
        got = run([(n, clauses)], [hint], None, None, 8)
        proved([(n, clauses)], [hint], None, got, want, [8])
        assert len(got['cube_status']) == 256 and int((got['cube_improvements'] > 0).sum()) <= 8
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    same_as_sequential(run([(n, clauses)], [None], None, None, 8), [sm.sequential(n, clauses, None, None, None, 0, 8)], 8)


def test_status_minus_three_among_good_instances(handle):
    inst, _, _, depth = sc.batch()
    hints, pens, begin = sc.dressed('start')
    good = run(inst, hints, pens, begin, depth, prob=handle)
    bad = [q.copy() for q in pens]
    hit = [5, 200, len(inst) - 3]
    bad[5][0] = -1
    bad[200][-1] = nc.CAP + 1
    bad[len(inst) - 3][7] = -(1 << 31)
    r = run(inst, hints, bad, begin, depth, prob=handle)
    promised(inst, hints, bad, r, depth)
    for i in hit:
        assert r['status'][i] == -3
        a, z = r['cube_off'][i], r['cube_off'][i + 1]
        assert (r['cube_status'][a:z] == 1).all() and not r['cube_work'][a:z].any() and (r['cube_cost'][a:z] == sm.NO_COST).all()
    rest = [i for i in range(len(inst)) if i not in hit]
    assert fields(r, rest) == fields(good, rest)


def fields(got, idx=None):
    "the promised fields in a comparable form"
    idx = range(len(got['status'])) if idx is None else idx
    return [(int(got['status'][j]), int(got['cost'][j]), int(got['depth_used'][j]), int(got['start_cost'][j]),
             int(got['cube_off'][j + 1] - got['cube_off'][j])) for j in idx]


def test_the_promised_fields_are_deterministic(handle):
    from pdp import native
    inst, _, _, depth = sc.batch()
    hints, pens, begin = sc.dressed('start')
    first = run(inst, hints, pens, begin, depth, prob=handle)
    a = fields(first)
    assert a == fields(run(inst, hints, pens, begin, depth, prob=handle))                 # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    pick = lambda per: [per[i] for i in order]
    shuffled = run(pick(inst), pick(hints), pick(pens), pick(begin), depth[order])        # a shuffled batch
    assert [a[i] for i in order] == fields(shuffled)
    promised(pick(inst), pick(hints), pick(pens), shuffled, depth[order])
    for i in list(range(0, len(inst), 31)) + [len(inst) - 1]:                             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            alone = run([inst[i]], [hints[i]], [pens[i]], [begin[i]], depth[i:i + 1])
            assert [a[i]] == fields(alone)
            promised([inst[i]], [hints[i]], [pens[i]], alone)
    prev = native.use_build('fast')
    try:
        fast = run(inst, hints, pens, begin, depth)
    finally:
        native.use_build(prev)
    assert a == fields(fast)
    promised(inst, hints, pens, fast, depth)


def test_one_handle_serves_both_optimising_split_calls(handle):
    "exact_nearest_split and exact_min_unsat_split interleaved: the setup block, the counter and the records of each are its own"
    inst, _, _, depth = sc.batch()
    hints, pens, _ = sc.dressed('mixed')
    d = torch.from_numpy(depth).cuda()
    h = flat(handle, inst, hints, np.float32, 0.0)
    a = fields(run(inst, hints, pens, None, depth, prob=handle))
    m1 = [t.cpu().numpy() for t in handle.exact_min_unsat_split(hints=h, depth=2, stats=True)]
    b = run(inst, hints, pens, None, depth, prob=handle)
    m2 = [t.cpu().numpy() for t in handle.exact_min_unsat_split(hints=h, depth=d, stats=True)]
    c = run(inst, hints, pens, None, 1, prob=handle)
    m3 = [t.cpu().numpy() for t in handle.exact_min_unsat_split(hints=h, depth=2, stats=True)]
    assert a == fields(b) and [x[:2] for x in a] == [x[:2] for x in fields(c)]
    promised(inst, hints, pens, b, depth)
    promised(inst, hints, pens, c, [1] * len(inst))
    assert (m1[0] == 1).all() and np.array_equal(m1[1], m2[1]) and np.array_equal(m1[1], m3[1]) and np.array_equal(m1[7], m3[7])
    assert np.array_equal(m2[6], depth) and (m3[6] == 2).all()


def test_refusals(tmp_path):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_nearest_split(depth=2, budget=1)
    p = native.Problem(*args)
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=p.device)
    cubes = (i64(p.B + 1), torch.empty(1 << 10, dtype=torch.int8, device=p.device), i64(1 << 10), i64(1 << 10),
             torch.empty(1 << 10, dtype=torch.int32, device=p.device))
    assert native.lib().pdp_exact_nearest_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK      # no split call yet
    # a call that must be refused runs with a budget of one read: should the refusal ever fail, its cubes end after one pass each
    for wrong, at in ((17, 5), (-1, 63)):
        depth = torch.zeros(p.B, dtype=torch.int8, device=p.device)
        depth[at] = wrong
        depth[70] = wrong
        with pytest.raises(native.NativeError, match='pdp_exact_nearest_split: the depth of instance %d is not in 0 .. 16' % at):
            p.exact_nearest_split(depth=depth, budget=1)
    with pytest.raises(native.NativeError, match=r'more than 2\^22 cubes in one call \(reached at instance 64\)'):
        p.exact_nearest_split(depth=16, budget=1)                                          # 80 * 2^16
    assert native.lib().pdp_exact_nearest_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK      # a refused call leaves none
    f32 = lambda k, **kw: torch.zeros(k, dtype=torch.float32, device=p.device, **kw)
    for wrong in (f32(p.V + 1), f32(p.V - 1), torch.zeros(p.V, dtype=torch.float64, device=p.device), np.zeros(p.V, dtype=np.float32),
                  torch.zeros(p.V, dtype=torch.float32)):
        with pytest.raises(ValueError):
            p.exact_nearest_split(hints=wrong, depth=2, budget=1)
        with pytest.raises(ValueError):
            p.exact_nearest_split(start=wrong, depth=2, budget=1)
    for wrong in (torch.ones(p.V + 1, dtype=torch.int32, device=p.device), torch.ones(p.V, dtype=torch.int64, device=p.device),
                  torch.ones(p.V, dtype=torch.float32, device=p.device), [1] * p.V, torch.ones(p.V, dtype=torch.int32)):
        with pytest.raises(ValueError):
            p.exact_nearest_split(penalties=wrong, depth=2, budget=1)
    for wrong in (1.5, '7', True, torch.zeros(p.B), torch.zeros(p.B - 1, dtype=torch.int8, device=p.device), torch.zeros(p.B, dtype=torch.int8)):
        with pytest.raises(ValueError):
            p.exact_nearest_split(depth=wrong, budget=1)
    with pytest.raises(ValueError):
        p.exact_nearest_split(budget=1.5)
    st = p.exact_nearest_split(depth=3)[0]
    assert set(st.cpu().numpy().tolist()) <= {0, 1}
    assert native.lib().pdp_exact_nearest_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) == native.PDP_OK
    items = dataset.random_ksat_items(2, 20, 3, seed=1)
    with pytest.raises(ValueError):
        exact.nearest_model(items, None, split=2, start=[np.zeros(20, dtype=np.float32), np.zeros(19, dtype=np.float32)])
    with pytest.raises(ValueError):
        exact.nearest_model(items, None, start=[np.zeros(20, dtype=np.float32)])
    for argv, said in ((['--complete', '--complete-nearest-split', '3'], 'give --complete-nearest as well'),
                       (['--complete', '--complete-nearest', '--complete-nearest-split', '17'], 'takes a depth from 0 to 16'),
                       (['--complete', '--complete-nearest', '--complete-nearest-split', '-2'], 'takes a depth from 0 to 16')):
        r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d'] + argv +
                           ['-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                           cwd=REPO)
        assert r.returncode != 0 and '--complete-nearest-split' in r.stderr and said in r.stderr


def test_nearest_model_split_on_segments_and_items_without_a_literal(monkeypatch):
    from pdp import exact
    few, fh, fp = [x[:100] for x in nc.small()]
    uni = nc.uniform()
    more = [k for k, (n, _) in enumerate(uni[0]) if n == 30]
    inst = few + [uni[0][k] for k in more]
    hints = [np.array([1, 0, np.nan], dtype=np.float32), None] + fh + [uni[1][k] for k in more] + [np.array([0.2, 0.9, 1, 0], dtype=np.float32)]
    pens = [None, None] + fp + [uni[2][k] for k in more] + [None]
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + [exact.raw_item(4, [[]])]
    base = exact.nearest_model(raw, hints, pens)
    assert set(base[0].tolist()) == {0, 1} and base[0][0] == 1 and base[0][1] == 0 and base[0][-1] == 0
    monkeypatch.setattr(exact, 'AUTO_NEAREST_STAGE1_BUDGET', 300)                         # so that the second stage has work to do
    seen, stage1 = [], []
    real, real_plain = exact.native.Problem.exact_nearest_split, exact.native.Problem.exact_nearest

    def spy(self, *a, **kw):
        out = real(self, *a, **kw)
        seen.append((a[2], out, len(stage1)))
        return out

    def spy_plain(self, *a, **kw):
        out = real_plain(self, *a, **kw)
        stage1.append(out)
        return out
    monkeypatch.setattr(exact.native.Problem, 'exact_nearest_split', spy)
    monkeypatch.setattr(exact.native.Problem, 'exact_nearest', spy_plain)
    for split in (4, 'auto'):
        for max_edges in (exact.MAX_EDGES, 400):
            del seen[:], stage1[:]
            got = exact.nearest_model(raw, hints, pens, split=split, max_edges=max_edges, depths=True)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
            assert (got[0].dtype, got[1].dtype, got[3].dtype, got[4].dtype) == (np.int8, np.int64, np.int64, np.int8)
            for (n, c), h, q, m, co, st in zip(inst, hints[2:-1], pens[2:-1], got[2][2:-1], got[1][2:-1], got[0][2:-1]):
                assert m.dtype == np.float32 and len(m) == n
                assert (st == 0 and co == -1) or (nc.satisfies(c, m) and nm.distance(nm.threshold(n, h), nm.penalty_list(n, q), m) == co)
            assert [m.tolist() for m in (got[2][0], got[2][1], got[2][-1])] == [[1, 0, 0], [0, 0], [0, 0, 0, 0]]
            assert got[3][0] == got[3][1] == got[3][-1] == 0
            if split == 4:
                assert (got[4][2:-1] == 4).all() and all(s is None for s, _, _ in seen)
            else:
                assert (got[4] > 0).sum() >= 5 and (got[4] == 0).sum() >= 5              # some rows end in the first stage, some do not
                assert (got[3][got[4] > 0] > 300).all()                                    # work is the sum of both stages
                # the start models carry over: where the first stage held a model, start_cost is its cost, which the kernel recomputed
                # inside the driver, instance by instance: the k-th row of the second stage is the k-th unproved row of the first stage
                # that came just before it, and where that row held a model its cost is the start_cost the kernel recomputed
                carried = 0
                for begin, out, at in seen:
                    assert begin is not None and at >= 1
                    st1, co1 = [t.cpu().numpy() for t in stage1[at - 1][:2]]
                    again = np.nonzero(st1 == -1)[0]
                    sc_, co_ = out[7].cpu().numpy(), out[1].cpu().numpy()
                    assert len(sc_) == len(again)
                    held = co1[again] >= 0
                    assert np.array_equal(sc_[held], co1[again][held])
                    assert ((sc_ == -1) | (co_ <= sc_)).all()
                    carried += int(held.sum())
                assert carried >= 1
    monkeypatch.setattr(exact.native.Problem, 'exact_nearest_split', real)
    monkeypatch.setattr(exact.native.Problem, 'exact_nearest', real_plain)
    # stage 1's cost is the start_cost of stage 2, instance by instance
    p = problem(inst)
    h, q = flat(p, inst, hints[2:-1], np.float32, 0.0), flat(p, inst, pens[2:-1], np.int32, 1)
    st1, co1, m1, _ = [t.cpu().numpy() for t in p.exact_nearest(h, q, 300)]
    r = p.exact_nearest_split(h, q, torch.from_numpy(m1).cuda(), depth=2, stats=True)
    held = (st1 == -1) & (co1 >= 0)
    assert held.sum() >= 2 and np.array_equal(r[7].cpu().numpy()[held], co1[held])
    np.testing.assert_array_equal(r[1].cpu().numpy(), base[1][2:-1])
    # a start model alone turns on the split call at depth 0
    with_start = exact.nearest_model(raw[2:12], hints[2:12], pens[2:12], start=[nc.any_model(n, c) for n, c in inst[:10]], depths=True)
    assert np.array_equal(with_start[1], base[1][2:12]) and not with_start[4].any()
    assert len(exact.nearest_model(raw[:5], hints[:5], pens[:5], split=2)) == 4


def test_cli_complete_nearest_split(tmp_path):
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
    own, _ = _run(argv[:-2], 1, str(tmp_path / 'own.jsonl'), 0)                          # PDP's own assignments: the hints
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-nearest-split', '3'], 1, str(tmp_path / 'deep.jsonl'), 0)
    auto, _ = _run(argv + ['--complete-nearest-split', '-1'], 1, str(tmp_path / 'auto.jsonl'), 0)
    assert len(base) == len(deep) == len(auto) == 40
    split = 0
    moved = ('nearest_solution', 'nearest_work', 'nearest_split_depth')
    for o, b, d, a in zip(own, base, deep, auto):
        r, rb, ra, o = json.loads(d), json.loads(b), json.loads(a), json.loads(o)
        if rb['complete'] != 1:
            assert d == b and a == b                                                     # byte-identical to the run without the flag
            continue
        assert list(r)[-2:] == ['nearest_work', 'nearest_split_depth'] and list(r)[:-1] == list(rb) and r['nearest_split_depth'] == 3
        assert {k: v for k, v in r.items() if k not in moved} == {k: v for k, v in rb.items() if k not in moved}
        assert rb['nearest_proved'] == 1 and r['nearest_work'] > 0
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        assert len(r['nearest_solution']) == n and nc.satisfies(clauses, r['nearest_solution'])
        assert r['nearest'] == sum(x != y for x, y in zip(r['nearest_solution'], o['solution']))
        # auto: every row is proved by the plain first stage, whose outputs are the plain call's
        assert list(ra) == list(rb) and ra == rb
        split += 1
    assert split >= 10
