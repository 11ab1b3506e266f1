"""The hinted complete search on the GPU (pdp_exact_solve_hinted, Problem.exact_solve(hints=), exact.solve_items(hints=)) and what is
built on it (SatFactorGraphTrainer._post_process_complete, satyr.py --complete): equal to its Python statement (tests/exact_model.py) in
status, model and work; the properties P1-P4 of the specification (include/pdp_hip.h) at a size with real backtracking; determinism,
budget, the HBM route, refusals; the trainer's rows and the command line."""
import ctypes
import io
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_model
from helpers import REPO
from test_exact_gpu import DEGENERATE, planted, random_instance, satisfies
from test_exact_host import brute_force, dpll

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')


def hsolve(instances, hints=None, budget=0):
    from pdp import exact
    return exact.solve_items([exact.raw_item(n, c) for n, c in instances], budget=budget, hints=hints)


def same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    assert all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))


def random_hints(rng, inst, nan=0.0):
    out = []
    for n, _ in inst:
        h = rng.randint(0, 2, size=n).astype(np.float32) if nan == 0.0 else rng.rand(n).astype(np.float32)
        if nan:
            h[rng.rand(n) < nan] = np.nan
        out.append(h)
    return out


def check_reads(inst, hints):
    return np.array([exact_model.check_reads(c, h)[0] for (_, c), h in zip(inst, hints)], dtype=np.int64)


@pytest.fixture(scope='module')
def small():
    "about 600 small instances, their unhinted GPU run, and three kinds of hints: random 0/1, random with 30 % NaN, the own model"
    rng = np.random.RandomState(35)                           # 144 satisfiable, 465 unsatisfiable (tests/exact_model.py on the CPU)
    inst = [random_instance(rng, 18) for _ in range(600)] + DEGENERATE
    plain = hsolve(inst)
    kinds = {'random': random_hints(rng, inst), 'nan30': random_hints(rng, inst, 0.3), 'own': [m.copy() for m in plain[1]]}
    return inst, plain, kinds


@pytest.fixture(scope='module')
def small_hinted(small):
    inst, _, kinds = small
    return {k: hsolve(inst, h) for k, h in kinds.items()}


def test_equal_to_the_python_model_exactly(small, small_hinted):
    inst, plain, kinds = small
    want = np.array([brute_force(n, c) for n, c in inst])
    assert int(want.sum()) >= 100 and int((~want).sum()) >= 100
    same(plain, exact_model.solve(inst))
    for k, hints in kinds.items():
        same(small_hinted[k], exact_model.solve(inst, hints))
        np.testing.assert_array_equal(small_hinted[k][0] == 1, want)


@pytest.fixture(scope='module')
def threshold():
    "the 100 threshold instances of test_exact_gpu.test_threshold_3sat_equals_python_dpll"
    rng = np.random.RandomState(77)
    inst = []
    for _ in range(100):
        clauses = []
        for _ in range(int(round(4.26 * 50))):
            vs = rng.choice(50, size=3, replace=False) + 1
            clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
        inst.append((50, clauses))
    return inst, hsolve(inst)


def test_properties_with_real_backtracking(threshold):
    inst, plain = threshold
    assert set(np.unique(plain[0])) == {0, 1}
    hints = random_hints(np.random.RandomState(78), inst)
    rnd = hsolve(inst, hints)
    np.testing.assert_array_equal(rnd[0], plain[0])                                          # P1
    unsat = plain[0] == 0
    np.testing.assert_array_equal(rnd[2][unsat], (plain[2] + check_reads(inst, hints))[unsat])   # P2
    assert all(satisfies(c, m) for (n, c), s, m in zip(inst, rnd[0], rnd[1]) if s == 1)
    own = hsolve(inst, [m.copy() for m in plain[1]])                                         # P3
    sat = plain[0] == 1
    np.testing.assert_array_equal(own[0], plain[0])
    assert all(np.array_equal(a, b) for a, b in zip(own[1], plain[1]))
    np.testing.assert_array_equal(own[2][sat], check_reads(inst, plain[1])[sat])
    assert (own[2][sat] <= plain[2][sat]).all()
    assert int((own[2][sat] < plain[2][sat]).sum()) >= 10


def small_problem(inst):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    b = dataset.to_torch(dataset.collate_segment([exact.raw_item(n, c) for n, c in inst]), torch.device('cuda:0'))
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(inst))


def test_no_hints_is_the_unhinted_search(small):
    "P4: hints=None, a NULL pointer and an all-NaN tensor each give exact_solve()'s three outputs"
    from pdp import native
    p = small_problem(small[0])
    want = [t.cpu().numpy() for t in p.exact_solve()]
    status = torch.empty(p.B, dtype=torch.int8, device=p.device)
    model = torch.empty(p.V, dtype=torch.float32, device=p.device)
    work = torch.empty(p.B, dtype=torch.int64, device=p.device)
    native.check(native.lib().pdp_exact_solve_hinted(p._h, ctypes.c_void_p(0), ctypes.c_int64(0), native.ptr(status), native.ptr(model),
                                                     native.ptr(work), native._stream()))
    nan = torch.full((p.V,), float('nan'), dtype=torch.float32, device=p.device)
    for got in (p.exact_solve(hints=None), (status, model, work), p.exact_solve(hints=nan)):
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b.cpu().numpy())
    assert set(np.unique(want[0])) == {0, 1}


def test_deterministic_and_instance_local_with_hints(small, small_hinted):
    from pdp import native
    inst, _, kinds = small
    for k in ('random', 'nan30'):
        a, hints = small_hinted[k], kinds[k]
        same(a, hsolve(inst, hints))
        r = hsolve(inst[::-1], hints[::-1])
        same(a, (r[0][::-1], r[1][::-1], r[2][::-1]))
        for i in list(range(0, len(inst), 23)) + [len(inst) - 1]:
            s, m, w = hsolve([inst[i]], [hints[i]])
            assert s[0] == a[0][i] and w[0] == a[2][i] and np.array_equal(m[0], a[1][i]), i
    prev = native.use_build('fast')
    try:
        fast = {k: hsolve(inst, kinds[k]) for k in kinds}
    finally:
        native.use_build(prev)
    for k in kinds:
        same(small_hinted[k], fast[k])


def test_budget_with_hints():
    need = (4, [[1, 2], [-1, 2], [1, -2], [3, 4]])                # no unit clause: the unhinted search cannot decide it within budget 1
    good, bad = np.array([1, 1, 0, 1], dtype=np.float32), np.array([0, 0, 0, 0], dtype=np.float32)
    s, m, w = hsolve([need, need, need], [good, bad, None], budget=1)
    assert s.tolist() == [1, -1, -1]
    assert np.array_equal(m[0], good) and w[0] == exact_model.check_reads(need[1], good)[0] and w[2] > 0
    rng = np.random.RandomState(3)
    inst = [random_instance(rng, 18) for _ in range(400)]
    hints = random_hints(rng, inst)
    full = hsolve(inst, hints)
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    for budget in (50, 400, 3000):
        s, m, w = hsolve(inst, hints, budget=budget)
        assert (w < budget + 3 * edges).all()
        und = s == -1
        assert (w[und] >= budget).all()
        np.testing.assert_array_equal(s[~und], full[0][~und])
        np.testing.assert_array_equal(w[~und], full[2][~und])
        assert all(np.array_equal(m[i], full[1][i]) for i in np.nonzero(~und)[0])
        assert (full[2][und] >= budget).all()


def test_hints_on_the_hbm_route():
    "n = 1 600 at alpha 2: the slab (25 n + 2 e + 2 m bytes = 65 600) is past the 48 KiB of the LDS route"
    big = planted(1600, 2.0, 3, 9)
    big_unsat = (big[0], [[7]] + big[1] + [[-7]])
    rng = np.random.RandomState(4)
    few = [random_instance(rng, 12) for _ in range(50)]
    inst = few[:25] + [big] + few[25:] + [big_unsat]
    plain = hsolve(inst)
    assert plain[0][25] == 1 and plain[0][-1] == 0
    rnd = random_hints(rng, inst)
    own = [m.copy() for m in plain[1]]
    for hints in (rnd, own):
        got = hsolve(inst, hints)
        np.testing.assert_array_equal(got[0], plain[0])
        assert satisfies(big[1], got[1][25])
        unsat = plain[0] == 0
        np.testing.assert_array_equal(got[2][unsat], (plain[2] + check_reads(inst, hints))[unsat])
        alone = hsolve([big, big_unsat], [hints[25], hints[-1]])
        for j, i in enumerate((25, len(inst) - 1)):
            assert alone[0][j] == got[0][i] and alone[2][j] == got[2][i] and np.array_equal(alone[1][j], got[1][i])
    # P3 on the big instance
    assert np.array_equal(got[1][25], plain[1][25])
    assert got[2][25] == exact_model.check_reads(big[1], plain[1][25])[0] <= plain[2][25]


def test_refusals():
    from pdp import native
    from pdp.factorgraph import dataset
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(4, 20, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_solve(hints=torch.zeros(p.V, dtype=torch.float32, device=p.device))
    p = native.Problem(*args)
    for wrong in (torch.zeros(p.V + 1, dtype=torch.float32, device=p.device), torch.zeros(p.V - 1, dtype=torch.float32, device=p.device),
                  torch.zeros(p.V, dtype=torch.float64, device=p.device)):
        with pytest.raises(ValueError):
            p.exact_solve(hints=wrong)
    from pdp import exact
    with pytest.raises(ValueError):
        exact.solve_items(dataset.random_ksat_items(2, 20, 3, seed=1), hints=[np.zeros(20, dtype=np.float32), np.zeros(19, dtype=np.float32)])


FIVE = ['ID', 'label', 'solved', 'unsat_clauses', 'solution']


def item_clauses(it):
    rows = [[] for _ in range(int(it[1]))]
    for v, c, s in zip(it[2][0], it[2][1], it[3]):
        rows[int(c)].append((int(v) + 1) * int(s))
    return rows


@pytest.mark.parametrize('count,replication', [(1000, 1), (200, 3)])
def test_trainer_rows_are_completed(tmp_path, count, replication):
    "the set-up of test_exact_gpu.test_pdp_solved_instances_are_satisfiable, with and without _post_process_complete"
    from pdp import exact, generator
    from pdp.factorgraph import dataset
    from pdp.trainer import SatFactorGraphTrainer
    items = dataset.random_ksat_items(count, 50, 3, m=200, seed=123)
    path = tmp_path / 'n50.json'
    with open(str(path), 'w') as f:
        for it in items:
            sv = ((it[2][0] + 1) * it[3]).astype(int)
            f.write(generator.format_json_line(it[0], it[1], sv, it[2][1] + 1, label=-1, name=it[5][0]) + '\n')
    cfg = dict(model_type='p-d-p', model_name='complete', verbose=False, local_search_iteration=100, epsilon=0.5, tolerance=0.02,
               t_max=100, pi=0.01, decimation_probability=0.5, rng='philox', random_seed=0, hidden_dim=3, test_batch_limit=40000000,
               batch_size=5000, test_recurrence_num=100)
    tr = SatFactorGraphTrainer(cfg, use_cuda=True, logger=logging.getLogger('complete'))
    out = {}
    for name, post in (('plain', tr._post_process_predictions), ('complete', tr._post_process_complete)):
        buf = io.StringIO()
        tr.predict(str(path), buf, import_path_base=None, post_processor=post, batch_replication=replication)
        out[name] = [json.loads(l) for l in buf.getvalue().split('\n') if l.strip()]
        assert tr.last_stats['instances'] == count and tr.last_stats['solved'] == sum(r['solved'] for r in out[name])
        assert tr.last_stats['unsat_clauses'] == sum(r['unsat_clauses'] for r in out[name])
    plain, rows = out['plain'], out['complete']
    assert [r['ID'] for r in rows] == [r['ID'] for r in plain] == [it[5][0] for it in items]
    status, _, _ = exact.solve_items(items)
    assert all(list(r) == FIVE + ['complete', 'pdp_solved', 'work'] for r in rows) and all(list(r) == FIVE for r in plain)
    assert all(r['complete'] != -1 for r in rows)
    assert [r['complete'] for r in rows] == status.tolist()
    assert [r['pdp_solved'] for r in rows] == [r['solved'] for r in plain]
    if count == 1000:
        assert sum(r['pdp_solved'] for r in rows) > 100
    rescued = 0
    for r, q, it in zip(rows, plain, items):
        if r['pdp_solved'] == 1:
            assert r['complete'] == 1 and r['solution'] == q['solution']
        if r['complete'] == 1:
            assert r['solved'] == 1 and r['unsat_clauses'] == 0 and len(r['solution']) == it[0]
            assert satisfies(item_clauses(it), r['solution'])
            rescued += r['pdp_solved'] == 0
        else:
            assert {k: r[k] for k in FIVE} == q
        assert r['work'] > 0
    assert rescued >= 1


def test_cli_complete(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    from test_sharded_gpu import _run
    ddir = os.path.join(REPO, 'tests', 'golden', 'dimacs20')
    argv = [PDP_YAML, ddir, '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    one, log = _run(argv + ['-v'], 1, str(tmp_path / 'one.jsonl'), 0)
    rows = [json.loads(l) for l in one]
    assert len(rows) == 20
    for r in rows:
        assert list(r)[:5] == FIVE and list(r)[5:] == ['complete', 'pdp_solved', 'work']
        n, clauses = dimacs2json.parse_dimacs(os.path.join(ddir, r['ID']))
        assert r['complete'] == (1 if dpll(n, clauses) else 0), r['ID']
        if r['complete'] == 1:
            assert r['solved'] == 1 and satisfies(clauses, r['solution'])
    said = log[log.index('complete search:'):].split('\n')[0]
    assert said == 'complete search: satisfiable %d, unsatisfiable %d, undecided 0' % (sum(r['complete'] == 1 for r in rows),
                                                                                         sum(r['complete'] == 0 for r in rows))
    two, _ = _run(argv, 2, str(tmp_path / 'two.jsonl'), 29791)
    assert two == one
    r = subprocess.run([sys.executable, SATYR] + argv + ['--split-forward', '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=300, cwd=REPO)
    assert r.returncode != 0 and '--complete does not run together with --split-forward' in r.stderr
