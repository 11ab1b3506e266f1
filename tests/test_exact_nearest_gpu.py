"""The nearest-model search on the GPU (pdp_exact_nearest, Problem.exact_nearest, exact.nearest_model, satyr.py --complete
--complete-nearest): equal to its Python statement (tests/exact_nearest_model.py) in status, cost, model, work and improvements, the
consequences N1-N7 of the specification (include/pdp_hip.h) against brute force, the deciding and the counting search on the same handle,
the shapes at which a wave's chunks of 64 can go wrong, the budget, determinism over batch, handle, grid and build, the HBM route,
refusals, and the command line."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_nearest_cases as cs
import exact_nearest_model as nm
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')


@pytest.fixture(autouse=True)
def limit():
    "a hung kernel ends the test run with a traceback instead of holding the GPU"
    faulthandler.dump_traceback_later(240, exit=True)
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


def run(inst, hints=None, pens=None, budget=0, prob=None):
    "the five outputs of Problem.exact_nearest in the layout of exact_nearest_model.solve"
    p = problem(inst) if prob is None else prob
    out = p.exact_nearest(flat(p, inst, hints, np.float32, 0.0), flat(p, inst, pens, np.int32, 1), budget, stats=True)
    st, cost, model, work, imp = [t.cpu().numpy() for t in out]
    ends = np.cumsum([n for n, _ in inst])
    return st, cost, np.split(model, ends[:-1]), work, imp


def sizes(inst):
    return [max([n] + [abs(l) for c in cl for l in c]) for n, cl in inst]


@pytest.fixture(scope='module')
def world():
    "one problem of a few hundred instances, the GPU's answers with mixed penalties and without, and the handle"
    inst, hints, pens = cs.batch()
    assert sizes(inst) == [n for n, _ in inst]
    p = problem(inst)
    return inst, hints, pens, p, {True: run(inst, hints, pens, prob=p), False: run(inst, hints, None, prob=p)}


def test_equal_to_the_python_model_exactly(world):
    inst, hints, pens, _, got = world
    assert len(inst) > 400
    for mixed in (True, False):
        want = cs.results(mixed)
        cs.same(got[mixed], want)
        assert set(np.unique(want[0])) == {0, 1} and (want[3] < cs.READ_LIMIT).all()
        assert (want[4] >= 2).sum() > 10 and (want[4] == 0).sum() > 50


def test_n2_n3_models_costs_and_brute_force(world):
    "N2 against exact_solve on the same handle; N3 against brute force (n <= 12), the hinted search's model and enumerate_models"
    from pdp import exact
    inst, hints, pens, p, got = world
    decided = p.exact_solve()[0].cpu().numpy()
    assert set(np.unique(decided)) == {0, 1}
    hint_t = flat(p, inst, hints, np.float32, 0.0)
    hs, hmodel, _ = [t.cpu().numpy() for t in p.exact_solve(hints=hint_t)]
    hmodels = np.split(hmodel, np.cumsum([n for n, _ in inst])[:-1])
    small = len(cs.small()[0])
    few = list(range(0, small, 7))
    listed = dict(zip(few, exact.enumerate_models([exact.raw_item(*inst[i]) for i in few], 50)[0]))
    for mixed in (True, False):
        st, cost, models, _, _ = got[mixed]
        np.testing.assert_array_equal(st, decided)
        for i, (n, c) in enumerate(inst):
            bits = nm.threshold(n, hints[i])
            pen = nm.penalty_list(n, pens[i] if mixed else None)
            if st[i] == 0:
                assert cost[i] == -1 and not models[i].any()
                continue
            assert cs.satisfies(c, models[i]) and nm.distance(bits, pen, models[i]) == cost[i]
            assert hs[i] == 1 and cost[i] <= nm.distance(bits, pen, hmodels[i])
            if i < small:
                assert cost[i] == cs.brute(n, c, bits, pen)[0]
            if i in listed:
                for m in np.asarray(listed[i]).reshape(-1, n):
                    assert cs.satisfies(c, m) and cost[i] <= nm.distance(bits, pen, m)


def test_n1_a_hint_that_is_a_model(world):
    inst, _, pens, p, got = world
    st, cost, models, _, _ = got[True]
    sat = [i for i in range(len(inst)) if st[i] == 1]
    assert len(sat) > 200
    sub = [inst[i] for i in sat]
    q = problem(sub)
    own = [models[i] for i in sat]
    a = run(sub, own, [pens[i] for i in sat], prob=q)
    hs, hm, hw = [t.cpu().numpy() for t in q.exact_solve(hints=flat(q, sub, own, np.float32, 0.0))]
    assert (a[0] == 1).all() and (a[1] == 0).all() and (a[4] == 0).all() and (hs == 1).all()
    assert all(np.array_equal(m, o) for m, o in zip(a[2], own))
    np.testing.assert_array_equal(a[3], hw)


def test_n4_work_against_the_count_on_the_same_handle(world):
    inst, _, _, p, got = world
    cst, _, _, cwork = [t.cpu().numpy() for t in p.exact_count()]
    done = cst == 1
    assert done.sum() > 400
    for mixed in (True, False):
        assert (got[mixed][3][done] <= cwork[done] + cs.edges(inst)[done]).all()


def test_n5_n6_zero_and_scaled_penalties(world):
    inst, hints, pens, p, got = world
    zero = run(inst, hints, [np.zeros(n, dtype=np.int32) for n, _ in inst], prob=p)
    sat = got[True][0] == 1
    assert (zero[1][sat] == 0).all() and (zero[4][sat] <= 1).all() and (zero[0] == got[True][0]).all()
    assert all(cs.satisfies(inst[i][1], zero[2][i]) for i in np.nonzero(sat)[0])
    plain = run(inst, hints, [np.minimum(q, 7) for q in pens], prob=p)
    for c in (3, 149796):                                                                    # 7 * 149796 <= 2^20
        scaled = run(inst, hints, [np.minimum(q, 7) * c for q in pens], prob=p)
        np.testing.assert_array_equal(scaled[1], np.where(plain[1] >= 0, plain[1] * c, plain[1]))
        cs.same((plain[0], plain[1], plain[2], plain[3], plain[4]), (scaled[0], plain[1], scaled[2], scaled[3], scaled[4]))


def test_n7_budget(world):
    inst, hints, pens, p, got = world
    full = got[True]
    edges = cs.edges(inst)
    last = None
    for budget in (1, 2000, 50000):
        st, cost, models, work, imp = run(inst, hints, pens, budget, prob=p)
        print('budget %d: status histogram %s, work max %d' % (budget, np.bincount(st + 1).tolist(), int(work.max())))
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all()
        none = (st == -1) & (cost == -1)
        assert all(not models[i].any() for i in np.nonzero(none | (st == 0))[0])
        for i in np.nonzero(cost >= 0)[0]:
            n, c = inst[i]
            assert cs.satisfies(c, models[i]) and nm.distance(nm.threshold(n, hints[i]), nm.penalty_list(n, pens[i]), models[i]) == cost[i]
        assert (cost[cost >= 0] >= full[1][cost >= 0]).all() and (cost[st != -1] == full[1][st != -1]).all()
        if last is not None:
            both = (last >= 0)
            assert (cost[both] >= 0).all() and (cost[both] <= last[both]).all()              # a status -1 cost never rises
        last = cost
        if budget == 1:
            checked = full[4] == 0                                                          # the check pass runs before the first budget check
            assert (st[checked & (full[0] == 1)] == 1).all() and (st[~checked & (edges > 0)] == -1).all()
        cs.same((st, cost, models, work, imp), cs.results(True, budget))
    assert (st == -1).any()


def test_deterministic_and_instance_local(world, monkeypatch):
    from pdp import native
    inst, hints, pens, p, got = world
    a = got[True]
    cs.same(a, run(inst, hints, pens, prob=p))                                              # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    r = run([inst[i] for i in order], [hints[i] for i in order], [pens[i] for i in order])  # a shuffled batch
    cs.same(cs.pick(a, order), r)
    for i in list(range(0, len(inst), 53)) + [len(inst) - 1]:                               # alone
        if cs.edges([inst[i]])[0] > 0:
            cs.same(cs.pick(a, [i]), run([inst[i]], [hints[i]], [pens[i]]))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                               # one wave takes every instance, one after the other
    one = run(inst, hints, pens, prob=p)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    cs.same(a, one)
    run(inst, hints, pens, prob=p)
    assert p.exact_last_grid() == len(inst)
    prev = native.use_build('fast')
    try:
        fast = run(inst, hints, pens)
    finally:
        native.use_build(prev)
    cs.same(a, fast)


def test_chunks_of_a_wave():
    "150 units against the hint on one level, 4 100 units of 2^20 each (the sum passes 2^32), more than 64 free variables with a true hint"
    cases = [cs.fan_case(150), cs.units_case(4100), cs.fill_case(100)]
    inst, hints, pens = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    got = run(inst, hints, pens)
    cs.same(got, nm.solve(inst, hints, pens))
    assert got[0].tolist() == [1, 1, 1] and got[1].tolist() == [150, 4100 << 20, 5]
    assert got[2][2][12:].all() and len(got[2][2]) == 112
    cs.same(cs.pick(got, [1]), run(inst[1:2], hints[1:2], pens[1:2]))


def test_wide_instances():
    "trails past 128, passes of 100 units, levels of more than 64 entries undone (test_exact_nearest_host.py asserts the widths)"
    inst, hints, pens = cs.wide_batch()
    want, _ = cs.wide_results()
    cs.same(run(inst, hints, pens, cs.WIDE_BUDGET), want)


def test_hbm_route():
    "section 9.8's instance past the slab inside a batch of small ones: equal to brute force and to the model, and the same alone"
    big, hint, pen = cs.slab_case()
    few, fh, fp = [x[:40] for x in cs.small()]
    inst, hints, pens = few[:20] + [big] + few[20:], fh[:20] + [hint] + fh[20:], fp[:20] + [pen] + fp[20:]
    got = run(inst, hints, pens)
    want = cs.slab_result()
    assert (got[0][20], got[1][20], got[3][20], got[4][20]) == (want[0], want[1], want[3], want[4]) and np.array_equal(got[2][20], want[2])
    assert got[1][20] == cs.brute(*big, nm.threshold(10, hint), pen)[0]
    rest = [i for i in range(len(inst)) if i != 20]
    cs.same(cs.pick(got, rest), cs.pick(cs.results(True), list(range(40))))
    cs.same(cs.pick(got, [20]), run([big], [hint], [pen]))


def test_status_minus_three_among_good_instances(world):
    inst, hints, pens, p, got = world
    bad = [q.copy() for q in pens]
    hit = [5, 200, len(inst) - 3]
    bad[5][0] = -1
    bad[200][-1] = cs.CAP + 1
    bad[len(inst) - 3][7] = -(1 << 31)
    r = run(inst, hints, bad, prob=p)
    rest = [i for i in range(len(inst)) if i not in hit]
    cs.same(cs.pick(r, rest), cs.pick(got[True], rest))
    for i in hit:
        assert (r[0][i], r[1][i], r[3][i], r[4][i]) == (-3, 0, 0, 0) and not r[2][i].any()


def test_refusals(tmp_path):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(4, 20, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_nearest()
    p = native.Problem(*args)
    f32 = lambda k, **kw: torch.zeros(k, dtype=torch.float32, device=p.device, **kw)
    for wrong in (f32(p.V + 1), f32(p.V - 1), torch.zeros(p.V, dtype=torch.float64, device=p.device), np.zeros(p.V, dtype=np.float32),
                  torch.zeros(p.V, dtype=torch.float32)):
        with pytest.raises(ValueError):
            p.exact_nearest(hints=wrong)
    for wrong in (torch.ones(p.V + 1, dtype=torch.int32, device=p.device), torch.ones(p.V, dtype=torch.int64, device=p.device),
                  torch.ones(p.V, dtype=torch.float32, device=p.device), [1] * p.V, torch.ones(p.V, dtype=torch.int32)):
        with pytest.raises(ValueError):
            p.exact_nearest(penalties=wrong)
    with pytest.raises(ValueError):
        p.exact_nearest(budget=1.5)
    lib = native.lib()
    import ctypes as C
    out = [torch.zeros(p.B, dtype=torch.int8, device=p.device), torch.zeros(p.B, dtype=torch.int64, device=p.device), f32(p.V)]
    for k in range(3):                                                                       # NULL status, cost or model: before any launch
        ptrs = [C.c_void_p(0) if j == k else C.c_void_p(t.data_ptr()) for j, t in enumerate(out)]
        assert lib.pdp_exact_nearest(p._h, None, None, C.c_int64(0), ptrs[0], ptrs[1], ptrs[2], None, None, None) == 1
    items = dataset.random_ksat_items(2, 20, 3, seed=1)
    with pytest.raises(ValueError):
        exact.nearest_model(items, [np.zeros(20, dtype=np.float32), np.zeros(19, dtype=np.float32)])
    with pytest.raises(ValueError):
        exact.nearest_model(items, None, penalties=[np.ones(20), None])
    r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d', '--complete-nearest',
                        '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                       cwd=REPO)
    assert r.returncode != 0 and '--complete-nearest' in r.stderr and 'give --complete as well' in r.stderr


def test_nearest_model_on_cut_segments_and_literal_free_items():
    from pdp import exact
    items = [exact.raw_item(3, []), exact.raw_item(2, [[], []]), exact.raw_item(4, [[]]), exact.raw_item(2, [])]
    st, cost, models, work = exact.nearest_model(items, [np.array([1, 0, np.nan], dtype=np.float32), None, np.array([0.2, 0.9, 1, 0], dtype=np.float32),
                                                         None], penalties=[None, None, None, np.array([-1, 0])])
    assert st.tolist() == [1, 0, 0, -3] and cost.tolist() == [0, -1, -1, 0] and work.tolist() == [0, 0, 0, 0]
    assert [m.tolist() for m in models] == [[1, 0, 0], [0, 0], [0, 0, 0, 0], [0, 0]]
    # inside a problem the kernel gives the same answers, and a cut along max_edges changes nothing
    inst, hints, pens = [x[:60] for x in cs.small()]
    raw = [exact.raw_item(n, c) for n, c in inst]
    whole, cut = exact.nearest_model(raw, hints, pens), exact.nearest_model(raw, hints, pens, max_edges=100)
    want = cs.pick(cs.results(True), list(range(60)))
    for r in (whole, cut):
        for k in (0, 1, 3):
            np.testing.assert_array_equal(r[k], want[k])
            assert r[k].dtype == want[k].dtype
        assert all(np.array_equal(a, b) for a, b in zip(r[2], want[2]))
    plain = exact.nearest_model(raw, hints)
    np.testing.assert_array_equal(plain[1], cs.results(False)[1][:60])
    # a soft prediction through map_penalties: the most probable model, against brute force in float64
    rng = np.random.RandomState(17)
    soft = [np.round(rng.rand(n), 3) for n, _ in inst]
    hp = [exact.map_penalties(w) for w in soft]
    st, cost, models, _ = exact.nearest_model(raw, [h for h, _ in hp], [q for _, q in hp])
    for i, (n, c) in enumerate(inst):
        best, _ = cs.brute(n, c, hp[i][0], hp[i][1])
        assert (st[i] == 0 and best is None) or (st[i] == 1 and cost[i] == best)


def test_cli_complete_nearest(tmp_path):
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
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    own, _ = _run(argv[:-1], 1, str(tmp_path / 'own.jsonl'), 0)                          # PDP's own assignments: the hints
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    got, log = _run(argv + ['--complete-nearest', '-v'], 1, str(tmp_path / 'near.jsonl'), 0)
    assert len(base) == len(got) == 40
    new = ['nearest', 'nearest_proved', 'nearest_solution', 'nearest_work']
    asked = proved = far = 0
    for o, b, g in zip(own, base, got):
        r, o = json.loads(g), json.loads(o)
        assert o['ID'] == r['ID']
        if r['complete'] != 1:
            assert g == b                                                                # byte-identical to the run without the flag
            continue
        assert list(r)[-4:] == new and {k: v for k, v in r.items() if k not in new} == json.loads(b)
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        assert len(r['nearest_solution']) == n and cs.satisfies(clauses, r['nearest_solution'])
        assert r['nearest_proved'] == 1 and r['nearest_work'] > 0
        assert (r['nearest'] == 0) == (r['pdp_solved'] == 1)
        if r['pdp_solved'] == 1:
            assert r['nearest_solution'] == r['solution'] == o['solution']
        assert r['nearest'] == sum(a != b for a, b in zip(r['nearest_solution'], o['solution']))
        assert r['nearest'] <= sum(a != b for a, b in zip(r['solution'], o['solution']))     # N3: the hinted search's model is a model we know
        asked += 1
        proved += r['nearest_proved']
        far += r['nearest'] > 0
    assert asked >= 10 and far >= 1
    said = log[log.index('complete search:'):].split('\n')[0]
    assert said.endswith('; nearest model proved for %d of %d' % (proved, asked))
