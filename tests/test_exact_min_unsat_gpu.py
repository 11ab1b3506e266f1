"""The optimising complete search on the GPU (pdp_exact_min_unsat, Problem.exact_min_unsat, exact.min_unsat, satyr.py --complete
--complete-min-unsat): equal to its Python statement (tests/exact_min_unsat_model.py) in status, cost, model, work and improvements, the
cost against brute force, the library's own evaluator and the deciding search, property M1, the budget, determinism over batch, handle,
grid and build, instances wider than a wave, the HBM route, refusals, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_min_unsat_cases as cs
import exact_min_unsat_model as mm
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')


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


def run(inst, hints=None, budget=0, prob=None):
    "the five outputs of Problem.exact_min_unsat in the layout of exact_min_unsat_model.solve"
    p = problem(inst) if prob is None else prob
    st, cost, model, work, imp = [t.cpu().numpy() for t in p.exact_min_unsat(budget, hints=hint_tensor(p, inst, hints), stats=True)]
    ends = np.cumsum([n for n, _ in inst])
    return st, cost, np.split(model, ends[:-1]), work, imp


def same(a, b):
    for i in (0, 1, 3, 4):
        np.testing.assert_array_equal(a[i], b[i])
        assert a[i].dtype == b[i].dtype
    assert len(a[2]) == len(b[2]) and all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))


def pick(res, idx):
    return tuple([res[k][i] for i in idx] if k == 2 else res[k][idx] for k in range(5))


@pytest.fixture(scope='module')
def small():
    "about 600 small instances with three kinds of hints, the model's answers and the GPU's"
    inst, kinds = cs.family(35, 600, 18)
    want = {k: mm.solve(inst, kinds[k]) for k in cs.KINDS}
    p = problem(inst)
    got = {k: run(inst, None if k == 'none' else kinds[k], prob=p) for k in cs.KINDS}
    return inst, kinds, want, got, p


def test_equal_to_the_python_model_exactly(small):
    inst, kinds, want, got, _ = small
    few = [i for i, (n, _) in enumerate(inst) if n <= 12]
    brute = np.array([cs.brute_min(*inst[i]) for i in few])
    assert len(few) > 300
    for k in cs.KINDS:
        same(got[k], want[k])
        assert (got[k][0] == 1).all()
        np.testing.assert_array_equal(got[k][1][few], brute)
        assert all(mm.unsat_count(c, m) == co for (_, c), m, co in zip(inst, got[k][2], got[k][1]))
    assert int((got['random'][4] > 0).sum()) > 100 and int((got['random'][4] == 0).sum()) > 20


def test_cost_zero_exactly_where_the_deciding_search_answers_one(small):
    "on the whole family -- empty clauses and instances without clauses included -- and under each kind of hints, on the fixture's handle"
    inst, _, _, got, p = small
    decided = p.exact_solve()[0].cpu().numpy()
    assert set(np.unique(decided)) == {0, 1}
    for k in cs.KINDS:
        np.testing.assert_array_equal(got[k][1] == 0, decided == 1)


def test_cost_against_cnf_eval_and_the_deciding_search(small):
    "pdp_cnf_eval's unsatisfied-clause count of the returned model, on the same handle, is the cost; cost 0 exactly where exact_solve says 1"
    inst, kinds, _, got, _ = small
    keep = [i for i, (n, c) in enumerate(inst) if len(c) > 0 and all(len(x) > 0 for x in c)]
    sub = [inst[i] for i in keep]
    p = problem(sub)
    for k in ('random', 'nan30'):
        st, cost, model, _ = p.exact_min_unsat(hints=hint_tensor(p, sub, [kinds[k][i] for i in keep]))
        solved, unsat = p.cnf_eval(model)
        np.testing.assert_array_equal(unsat.cpu().numpy().reshape(-1).astype(np.int64), cost.cpu().numpy().astype(np.int64))
        np.testing.assert_array_equal(cost.cpu().numpy(), got[k][1][keep])
        decided = p.exact_solve()[0].cpu().numpy()
        assert set(np.unique(decided)) == {0, 1}
        np.testing.assert_array_equal(cost.cpu().numpy() == 0, decided == 1)
        np.testing.assert_array_equal(solved.cpu().numpy().reshape(-1) == 1, decided == 1)


def test_m1_work_is_the_hinted_search_s():
    "100 instances of 3-SAT n = 50, m = 213; the hint is exact_solve's model of the instance without its last clause (zeros where it has none)"
    rng = np.random.RandomState(213)
    inst = [cs.threshold_3sat(rng, 50, 213) for _ in range(100)]
    less = problem([(n, c[:-1]) for n, c in inst])
    st, hint, _ = less.exact_solve()
    ok = np.nonzero(st.cpu().numpy() == 1)[0]
    assert len(ok) >= 20
    p = problem(inst)
    first = np.array([mm.unsat_count(c, h) for (_, c), h in zip(inst, np.split(hint.cpu().numpy(), 100))])
    assert (first[ok] <= 1).all() and (first[ok] == 1).any()
    ds, _, dw = [t.cpu().numpy() for t in p.exact_solve(hints=hint)]
    ms, cost, _, mw = [t.cpu().numpy() for t in p.exact_min_unsat(hints=hint)]
    np.testing.assert_array_equal(mw[ok], dw[ok])
    np.testing.assert_array_equal(cost[ok], np.where(ds[ok] == 1, 0, first[ok]))
    assert (ms[ok] == 1).all() and (ds[ok] == 0).any() and ((ds[ok] == 1) & (first[ok] == 1)).any()


def test_budget():
    rng = np.random.RandomState(184)
    inst = [cs.threshold_3sat(rng, 40, 184) for _ in range(60)]
    hints = cs.hints_of(rng, inst, 'random')
    first = np.array([mm.unsat_count(c, h) for (_, c), h in zip(inst, hints)])
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    last = None
    for budget in (1, 2000, 50000):
        st, cost, models, work, imp = run(inst, hints, budget, prob=p)
        print('budget %d: proved %d of %d, cost sum %d, work max %d' % (budget, int((st == 1).sum()), len(inst), int(cost.sum()), int(work.max())))
        assert set(np.unique(st)) <= {-1, 1}
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all()
        assert all(mm.unsat_count(c, m) == co for (_, c), m, co in zip(inst, models, cost))       # also under status -1
        assert (cost <= first).all()
        assert last is None or (cost <= last).all()
        last = cost
        if budget == 1:
            assert (first > 0).all() and (st == -1).all() and (imp == 0).all()
            assert all(np.array_equal(m, h) for m, h in zip(models, hints))                     # the hint itself
        if budget == 2000:
            same((st, cost, models, work, imp), mm.solve(inst, hints, budget))
    assert (st == -1).any() or (cost < first).any()


def test_deterministic_and_instance_local(small, monkeypatch):
    from pdp import native
    inst, kinds, _, got, p = small
    hints = kinds['nan30']
    a = got['nan30']
    same(a, run(inst, hints, prob=p))                                                   # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    r = run([inst[i] for i in order], [hints[i] for i in order])                        # a shuffled batch
    same(pick(a, order), r)
    for i in list(range(0, len(inst), 41)) + [len(inst) - 1]:                           # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            same(pick(a, [i]), run([inst[i]], [hints[i]]))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                           # one wave takes every instance, one after the other
    one = run(inst, hints, prob=p)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    same(a, one)
    run(inst, hints, prob=p)
    assert p.exact_last_grid() == len(inst)
    prev = native.use_build('fast')
    try:
        fast = run(inst, hints)
    finally:
        native.use_build(prev)
    same(a, fast)


def test_wide_instances():
    "n > 128, m > 128, optimum 2 by construction, a hint of cost 3: widths past one wave (test_exact_min_unsat_host.py asserts them)"
    inst, hints, want = [], [], []
    for F in cs.WIDE_F:
        (i, h), (res, _) = cs.wide(F), cs.wide_results(F)
        inst.append(i); hints.append(h); want.append(res)
    got = run(inst, hints)
    for j, w in enumerate(want):
        assert (got[0][j], got[1][j], got[3][j], got[4][j]) == (w[0], w[1], w[3], w[4]) and np.array_equal(got[2][j], w[2])
    assert got[1].tolist() == [2, 2] and (got[4] >= 1).all()
    same(pick(got, [1]), run(inst[1:], hints[1:]))


def test_hbm_route():
    "an instance past the slab inside a batch of small ones: equal to brute force and to the model, and the same alone"
    big, hint = cs.past_the_slab()
    rng = np.random.RandomState(4)
    from test_exact_gpu import random_instance
    few = [random_instance(rng, 12) for _ in range(40)]
    fh = cs.hints_of(rng, few, 'random')
    inst, hints = few[:20] + [big] + few[20:], fh[:20] + [hint] + fh[20:]
    got = run(inst, hints)
    want = cs.slab_result()
    assert (got[0][20], got[1][20], got[3][20], got[4][20]) == (want[0], want[1], want[3], want[4]) and np.array_equal(got[2][20], want[2])
    assert got[1][20] == cs.brute_min(*big) and mm.unsat_count(big[1], got[2][20]) == got[1][20]
    rest = [i for i in range(len(inst)) if i != 20]
    np.testing.assert_array_equal(got[1][rest], [cs.brute_min(*inst[i]) for i in rest])
    same(pick(got, [20]), run([big], [hint]))


def test_refusals(tmp_path):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(4, 20, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_min_unsat()
    p = native.Problem(*args)
    for wrong in (torch.zeros(p.V + 1, dtype=torch.float32, device=p.device), torch.zeros(p.V - 1, dtype=torch.float32, device=p.device),
                  torch.zeros(p.V, dtype=torch.float64, device=p.device), np.zeros(p.V, dtype=np.float32)):
        with pytest.raises(ValueError):
            p.exact_min_unsat(hints=wrong)
    with pytest.raises(ValueError):
        exact.min_unsat(dataset.random_ksat_items(2, 20, 3, seed=1), hints=[np.zeros(20, dtype=np.float32), np.zeros(19, dtype=np.float32)])
    r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d', '--complete-min-unsat',
                        '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                       cwd=REPO)
    assert r.returncode != 0 and '--complete-min-unsat' in r.stderr and 'give --complete as well' in r.stderr


def test_host_answers_segments_without_a_literal():
    from pdp import exact
    items = [exact.raw_item(3, []), exact.raw_item(2, [[], []]), exact.raw_item(4, [[]])]
    st, cost, models, work = exact.min_unsat(items, hints=[np.array([1, 0, np.nan], dtype=np.float32), None, np.array([0.2, 0.9, 1, 0], dtype=np.float32)])
    assert st.tolist() == [1, 1, 1] and cost.tolist() == [0, 2, 1] and work.tolist() == [0, 0, 0]
    assert [m.tolist() for m in models] == [[1, 0, 0], [0, 0], [0, 1, 1, 0]]
    # and through the cut along max_edges: the same answers as one problem
    rng = np.random.RandomState(9)
    from test_exact_gpu import random_instance
    inst = [random_instance(rng, 10) for _ in range(30)]
    hints = cs.hints_of(rng, inst, 'random')
    raw = [exact.raw_item(n, c) for n, c in inst]
    whole, cut = exact.min_unsat(raw, hints=hints), exact.min_unsat(raw, hints=hints, max_edges=100)
    for k in (0, 1, 3):
        np.testing.assert_array_equal(whole[k], cut[k])
    assert all(np.array_equal(a, b) for a, b in zip(whole[2], cut[2]))
    np.testing.assert_array_equal(whole[1], [cs.brute_min(n, c) for n, c in inst])


def test_cli_complete_min_unsat(tmp_path):
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
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    got, log = _run(argv + ['--complete-min-unsat', '-v'], 1, str(tmp_path / 'min.jsonl'), 0)
    assert len(base) == len(got) == 40
    new = ['min_unsat', 'min_unsat_proved', 'min_unsat_solution', 'min_unsat_work']
    asked = proved = 0
    for b, g in zip(base, got):
        r = json.loads(g)
        if r['complete'] == 1:
            assert g == b                                                                # byte-identical to the run without the flag
            continue
        assert list(r)[-4:] == new and {k: v for k, v in r.items() if k not in new} == json.loads(b)
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        assert r['complete'] == 0 and r['min_unsat'] >= 1
        assert r['min_unsat'] <= r['unsat_clauses']
        assert len(r['min_unsat_solution']) == n and mm.unsat_count(clauses, r['min_unsat_solution']) == r['min_unsat']
        assert r['min_unsat_proved'] in (0, 1) and r['min_unsat_work'] > 0
        asked += 1
        proved += r['min_unsat_proved']
    assert asked >= 5
    said = log[log.index('complete search:'):].split('\n')[0]
    assert said.endswith('; minimum unsatisfied clauses proved for %d of %d' % (proved, asked))
