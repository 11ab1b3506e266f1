"""The split complete search on the GPU (pdp_exact_solve_split, Problem.exact_solve_split, exact.solve_items(split=), satyr.py --complete
--complete-split): equal to its Python statement (tests/exact_split_model.py) in status, model, work, first, depth_used and the records of
the cubes up to first; depth 0 equal to exact_solve; status and model equal to exact_solve at every depth; the budget per cube;
determinism of everything promised over call, batch, grid and build; the HBM route; refusals; the host entry points; the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_split_model as sm
from exact_min_unsat_cases import threshold_3sat
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


def flat(inst, hints):
    "one float32 device tensor of all hints (NaN for an instance without any), or None"
    if hints is None:
        return None
    parts = [np.full(n, np.nan, dtype=np.float32) if h is None else np.asarray(h, dtype=np.float32) for (n, _), h in zip(inst, hints)]
    return torch.from_numpy(np.concatenate(parts)).cuda()


def run(inst, depth, hints=None, budget=0, prob=None):
    "Problem.exact_solve_split(stats=True) as a dict of numpy arrays, the model cut per instance"
    p = problem(inst) if prob is None else prob
    d = depth if isinstance(depth, int) else torch.from_numpy(np.asarray(depth, dtype=np.int8)).cuda()
    out = [t.cpu().numpy() for t in p.exact_solve_split(budget, hints=flat(inst, hints), depth=d, stats=True)]
    got = dict(zip(('status', 'model', 'work', 'first', 'depth_used', 'cube_off', 'cube_status', 'cube_work'), out))
    assert (got['status'].dtype, got['model'].dtype, got['work'].dtype, got['first'].dtype, got['depth_used'].dtype) == \
        (np.int8, np.float32, np.int64, np.int32, np.int8)
    assert got['cube_off'][0] == 0 and np.array_equal(np.diff(got['cube_off']), 1 << got['depth_used'].astype(np.int64))
    assert got['cube_status'].shape == got['cube_work'].shape == (got['cube_off'][-1],)
    got['model'] = np.split(got['model'], np.cumsum([n for n, _ in inst])[:-1])
    return got


def reference(inst, depth, hints=None, budget=0):
    depth = [depth] * len(inst) if isinstance(depth, int) else depth
    return [sm.search(n, c, None if hints is None else hints[i], budget, int(depth[i])) for i, (n, c) in enumerate(inst)]


def same_as_model(got, want, depth):
    "every promised output against tests/exact_split_model.py; the cubes above first only for what cannot depend on timing"
    depth = [depth] * len(want) if isinstance(depth, int) else depth
    for j, (st, model, work, first, cubes) in enumerate(want):
        assert (got['status'][j], got['work'][j], got['first'][j], got['depth_used'][j]) == (st, work, first, depth[j]), j
        assert np.array_equal(got['model'][j], model), j
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        cst, cwk = got['cube_status'][a:z], got['cube_work'][a:z]
        assert cst[:len(cubes)].tolist() == [c[0] for c in cubes] and cwk[:len(cubes)].tolist() == [c[1] for c in cubes], j
        if not cubes:                                       # the check pass accepted the hints: no cube is searched
            assert (cst == -2).all() and not cwk.any()
        assert set(np.unique(cst[len(cubes):])) <= {-2, -1, 0, 1}


def promised(got):
    "what must not depend on timing, in a comparable form: the five outputs and the records of the cubes up to first"
    rec = []
    for j, first in enumerate(got['first']):
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        last = a + int(first) + 1 if first >= 0 else z     # no model in any cube, or the hints accepted: every record is fixed
        rec.append((got['cube_status'][a:last].tolist(), got['cube_work'][a:last].tolist()))
    return [(int(got['status'][j]), got['model'][j].tolist(), int(got['work'][j]), int(got['first'][j]), int(got['depth_used'][j]), rec[j])
            for j in range(len(rec))]


def make_hints(rng, inst, kind):
    if kind == 'none':
        return None
    out = []
    for n, c in inst:
        n = max([n] + [abs(l) for cl in c for l in cl])
        h = rng.rand(n).astype(np.float32)
        if kind == 'nan':
            h[rng.rand(n) < 0.4] = np.nan
            out.append(None if rng.rand() < 0.1 else h)
        else:                                               # complete hints: every third instance gets a model of its own where it has one
            st, model, _ = sm.cube(n, c, None, 0, 0, 0) if rng.rand() < 0.34 else (0, None, 0)
            out.append(model.copy() if st == 1 else h)
    return out


@pytest.fixture(scope='module')
def batch():
    "the n <= 12 family and uniform 3-SAT of n = 20 / 30 / 40 at clause ratios 3.5 / 4.26 / 5.0 in one problem, depths mixed over 0..6"
    inst = cs.family() + cs.uniform_3sat(120, 20, (3.5, 4.26, 5.0), 3) + cs.uniform_3sat(130, 30, (3.5, 4.26, 5.0), 2) + \
        cs.uniform_3sat(140, 40, (3.5, 4.26, 5.0), 2)
    inst = [(max([n] + [abs(l) for cl in c for l in cl]), c) for n, c in inst]
    depth = np.random.RandomState(7).randint(0, 7, size=len(inst)).astype(np.int8)
    return inst, depth, problem(inst)


@pytest.mark.parametrize('kind', ['none', 'nan', 'complete'])
def test_equal_to_the_python_model_exactly(batch, kind):
    inst, depth, p = batch
    hints = make_hints(np.random.RandomState(11), inst, kind)
    want = reference(inst, depth, hints)
    got = run(inst, depth, hints, prob=p)
    accepted = sum(1 for w in want if not w[4])
    late = sum(1 for w in want if w[3] > 0)
    print('split %s: %d instances, %d cubes, accepted by the check pass %d, first > 0 on %d, stopped early %d'
          % (kind, len(inst), len(got['cube_status']), accepted, late, int((got['cube_status'] == -2).sum())))
    same_as_model(got, want, depth)
    assert late >= 3 and (accepted > 40 if kind == 'complete' else kind == 'nan' or accepted == 0)
    assert {w[0] for w in want} == {0, 1}
    # depth 0 on the same handle: exact_solve's three outputs, and the same status and model at the mixed depths
    plain = [t.cpu().numpy() for t in p.exact_solve(hints=flat(inst, hints))]
    zero = run(inst, 0, hints, prob=p)
    assert np.array_equal(zero['status'], plain[0]) and np.array_equal(np.concatenate(zero['model']), plain[1])
    assert np.array_equal(zero['work'], plain[2]) and not zero['depth_used'].any()
    assert np.array_equal(got['status'], plain[0]) and np.array_equal(np.concatenate(got['model']), plain[1])


def test_status_and_model_of_the_plain_search_at_n_100():
    rng = np.random.RandomState(100)
    inst = [threshold_3sat(rng, 100, 426) for _ in range(32)]
    p = problem(inst)
    st, model, work = [t.cpu().numpy() for t in p.exact_solve()]
    assert set(np.unique(st)) == {0, 1}
    for depth in (6, 10):
        got = run(inst, depth, prob=p)
        print('n=100 depth %d: work ratio to the plain search %.2f, cubes stopped early %d of %d'
              % (depth, got['work'].sum() / work.sum(), int((got['cube_status'] == -2).sum()), len(got['cube_status'])))
        assert np.array_equal(got['status'], st) and np.array_equal(np.concatenate(got['model']), model)
        assert (got['depth_used'] == depth).all() and ((got['first'] >= 0) == (st == 1)).all() and (got['first'] > 0).sum() >= 3
        assert p.exact_last_grid() > 32                     # more waves at work than instances


def test_budget_per_cube():
    inst = cs.family()[::5] + cs.uniform_3sat(184, 40, (3.5, 4.26, 4.6), 4)
    inst = [(max([n] + [abs(l) for cl in c for l in cl]), c) for n, c in inst]
    depth = np.random.RandomState(8).randint(0, 5, size=len(inst)).astype(np.int8)
    hints = make_hints(np.random.RandomState(12), inst, 'complete')
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    seen = set()
    for budget in (2000, 50000):
        for h in (None, hints):
            got = run(inst, depth, h, budget, prob=p)
            same_as_model(got, reference(inst, depth, h, budget), depth)
            assert (got['work'] < (1 << depth.astype(np.int64)) * (budget + 3 * edges)).all()
            assert (got['cube_work'] < budget + 3 * np.repeat(edges, 1 << depth.astype(np.int64))).all()
            seen |= set(got['status'].tolist())
    assert seen == {-1, 0, 1}


def test_deterministic_in_everything_promised(monkeypatch):
    from pdp import native
    rng = np.random.RandomState(77)
    easy = []                                                                             # satisfiable, first small among 1 024 cubes each
    while len(easy) < 6:
        n, c = threshold_3sat(rng, 40, 140)
        if sm.search(n, c, depth=10)[3] in range(64):
            easy.append((n, c))
    hard = cs.uniform_3sat(78, 40, (4.26, 5.0), 3)
    tiny = [(3, [[1, 2, 3], [-1, -2], [-2, -3], [2, 3]]), (3, [[1, 2], [-1, 2], [1, -2], [-1, -2], [3, 1]])]
    few = cs.family()[:60]
    inst = easy + hard + tiny + [(max([n] + [abs(l) for cl in c for l in cl]), c) for n, c in few]
    depth = np.array([10] * 6 + [4] * 6 + [8, 8] + list(np.random.RandomState(9).randint(0, 7, size=len(few))), dtype=np.int8)
    p = problem(inst)
    first = run(inst, depth, prob=p)
    a = promised(first)
    assert all(x[0] == 1 and 0 <= x[3] < 64 for x in a[:6]) and any(x[3] > 0 for x in a[:6])     # far more cubes above first than one grid holds
    plain = [t.cpu().numpy() for t in p.exact_solve()]
    assert np.array_equal(first['status'], plain[0]) and np.array_equal(np.concatenate(first['model']), plain[1])
    assert a == promised(run(inst, depth, prob=p))                                        # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    assert [a[i] for i in order] == promised(run([inst[i] for i in order], depth[order]))  # a shuffled batch
    for i in (0, 5, 7, 12, 13, 20, len(inst) - 1):                                        # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            assert [a[i]] == promised(run([inst[i]], depth[i:i + 1]))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every cube, one after the other:
    one = run(inst, depth, prob=p)                                                        # every cube above first sees best already set
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    assert a == promised(one)
    for j in range(6):                                                                    # ... and stops before it reads a clause
        z0, z1 = one['cube_off'][j] + one['first'][j] + 1, one['cube_off'][j + 1]
        assert (one['cube_status'][z0:z1] == -2).all() and not one['cube_work'][z0:z1].any()
    run(inst, depth, prob=p)
    assert p.exact_last_grid() > 1
    prev = native.use_build('fast')
    try:
        fast = run(inst, depth)
    finally:
        native.use_build(prev)
    assert a == promised(fast)


def test_hbm_route_is_searched_at_depth_zero():
    big = cs.past_the_slab()
    few = cs.family()[:40]
    inst = few[:20] + [big] + few[20:]
    inst = [(max([n] + [abs(l) for cl in c for l in cl]), c) for n, c in inst]
    p = problem(inst)
    got = run(inst, 3, prob=p)
    plain = [t.cpu().numpy() for t in p.exact_solve()]
    assert got['depth_used'][20] == 0 and (np.delete(got['depth_used'], 20) == 3).all()
    assert got['status'][20] == plain[0][20] == 1 and got['work'][20] == plain[2][20] and got['first'][20] == 0
    assert np.array_equal(got['status'], plain[0]) and np.array_equal(np.concatenate(got['model']), plain[1])
    alone = run([inst[20]], 3)
    assert alone['depth_used'].tolist() == [0] and alone['work'][0] == plain[2][20] and np.array_equal(alone['model'][0], got['model'][20])


def test_refusals(tmp_path):
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_solve_split(depth=2)
    p = native.Problem(*args)
    cubes = (torch.empty(p.B + 1, dtype=torch.int64, device=p.device), torch.empty(1 << 10, dtype=torch.int8, device=p.device),
             torch.empty(1 << 10, dtype=torch.int64, device=p.device))
    assert native.lib().pdp_exact_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK       # no split call yet
    for wrong, at in ((17, 5), (-1, 63)):
        depth = torch.zeros(p.B, dtype=torch.int8, device=p.device)
        depth[at] = wrong
        depth[70] = wrong
        with pytest.raises(native.NativeError, match='depth of instance %d is not in 0 .. 16' % at):
            p.exact_solve_split(depth=depth)
    with pytest.raises(native.NativeError, match=r'more than 2\^22 cubes in one call \(reached at instance 64\)'):
        p.exact_solve_split(depth=16)                                                       # 80 * 2^16
    ok = torch.zeros(p.B, dtype=torch.int8, device=p.device)
    ok[:63] = 16
    st = p.exact_solve_split(depth=ok)[0]                                                   # 63 * 2^16 + 17 cubes: within the limit
    assert set(st.cpu().tolist()) <= {0, 1}
    for wrong in (1.5, '7', True, torch.zeros(p.B), torch.zeros(p.B - 1, dtype=torch.int8, device=p.device), torch.zeros(p.B, dtype=torch.int8)):
        with pytest.raises(ValueError):
            p.exact_solve_split(depth=wrong)
    with pytest.raises(ValueError):
        p.exact_solve_split(hints=torch.zeros(3))
    r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d', '--complete-split', '3',
                        '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                       cwd=REPO)
    assert r.returncode != 0 and '--complete-split' in r.stderr and 'give --complete as well' in r.stderr
    r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d', '--complete',
                        '--complete-learn', '--complete-split', '3', '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=300, cwd=REPO)
    assert r.returncode != 0 and 'without --complete-learn and --complete-certify' in r.stderr


def test_solve_items_split_on_segments_and_items_without_a_literal(monkeypatch):
    from pdp import exact
    inst = cs.family()[:120] + cs.uniform_3sat(150, 30, (3.5, 4.26, 5.0), 3)
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + [exact.raw_item(4, [[]])]
    rng = np.random.RandomState(15)
    hints = [None if rng.rand() < 0.3 else rng.rand(int(it[0])).astype(np.float32) for it in raw]
    base = exact.solve_items(raw, hints=hints)
    assert set(base[0].tolist()) == {0, 1}
    monkeypatch.setattr(exact, 'AUTO_STAGE1_BUDGET', 300)                                 # so that the second stage has work to do
    for split in (4, 'auto'):
        for max_edges in (exact.MAX_EDGES, 400):
            got = exact.solve_items(raw, hints=hints, split=split, max_edges=max_edges)
            assert np.array_equal(got[0], base[0]) and got[0].dtype == np.int8 and got[2].dtype == np.int64
            assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(got[1], base[1]))
            assert (got[2] >= 0).all() and got[2][0] == got[2][1] == got[2][-1] == 0
    target = exact.AUTO_CUBES_PER_WAVE * torch.cuda.get_device_properties('cuda:0').multi_processor_count * 4 * exact.SPLIT_WAVES_PER_SIMD
    for undecided in (1, 8, 64, 5000, 10 ** 9):
        d = exact.auto_depth(undecided, 'cuda:0')
        assert 0 <= d <= 16 and (d == 0 or (undecided << d) <= target) and (d == 16 or target < (undecided << (d + 1)))
    assert exact.label_clause_lists([inst[0], inst[-1]], split='auto') == exact.label_clause_lists([inst[0], inst[-1]])
    assert exact.is_sat(*inst[-1], split=5) == exact.is_sat(*inst[-1])


def test_cli_complete_split(tmp_path):
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    for i in range(40):
        n, clauses = threshold_3sat(rng, 30, 128)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-split', '3'], 1, str(tmp_path / 'deep.jsonl'), 0)
    auto, _ = _run(argv + ['--complete-split', '-1'], 1, str(tmp_path / 'auto.jsonl'), 0)
    assert len(base) == len(deep) == len(auto) == 40
    split = 0
    for b, d in zip(base, deep):
        r = json.loads(d)
        if 'split_depth' not in r:
            assert d == b                                                                # byte-identical to the run without the flag
            continue
        assert r['split_depth'] == 3 and list(r)[list(r).index('work') + 1] == 'split_depth'
        assert {k: v for k, v in r.items() if k not in ('work', 'split_depth')} == {k: v for k, v in json.loads(b).items() if k != 'work'}
        assert r['work'] > 0
        split += 1
    assert split == 40
    assert auto == base                                                                   # every row is decided by the plain first stage
    assert {json.loads(b)['complete'] for b in base} == {0, 1}
