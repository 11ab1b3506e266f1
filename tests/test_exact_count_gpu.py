"""The counting complete search on the GPU (pdp_exact_count, Problem.exact_count, exact.count_models, satyr.py --complete
--complete-count): equal to its Python statement (tests/exact_count_model.py) bit for bit in status, count, true_count, work and leaves,
the counts against brute force, the deciding search and the backbone, the budget, determinism over batch, handle, grid and build, a level
wider than a wave, the HBM route, instances that are too large, refusals, and the command line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_count_model as cm
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


def run(inst, budget=0, prob=None):
    "the five outputs of Problem.exact_count in the layout of exact_count_model.solve"
    p = problem(inst) if prob is None else prob
    st, count, tc, work, leaves = [t.cpu().numpy() for t in p.exact_count(budget, stats=True)]
    ends = np.cumsum([n for n, _ in inst])
    return st, count, np.split(tc, ends[:-1]), work, leaves


N50_SEED = 53


@pytest.fixture(scope='module')
def batch():
    """about 500 instances in one problem: the host family (n <= 12), the two fans, uniform 3-SAT of n = 20 / 30 / 50 at clause ratios
    3.5, 4.0 and 4.5; the model's answers and the GPU's"""
    n50 = cs.uniform_3sat(N50_SEED, 50, (3.5, 4.0, 4.5), 3)
    want50 = cm.solve(n50)
    assert (want50[0] == 1).all() and (want50[3] < 1 << 22).all()                         # all finish under 2^22 reads
    rest = cs.family() + [cs.fan(k) for k in cs.FAN_K] + cs.uniform_3sat(20, 20, (3.5, 4.0, 4.5), 14) + cs.uniform_3sat(30, 30, (3.5, 4.0, 4.5), 12)
    part = cm.solve(rest)
    inst = rest + n50
    want = tuple(a + b if k == 2 else np.concatenate([a, b]) for k, (a, b) in enumerate(zip(part, want50)))
    p = problem(inst)
    return inst, want, run(inst, prob=p), p


def test_equal_to_the_python_model_exactly(batch):
    inst, want, got, _ = batch
    assert len(inst) >= 500
    print('count: %d instances, %d with models, leaves max %d, work max %d' % (len(inst), int((got[1] > 0).sum()), int(got[4].max()), int(got[3].max())))
    cs.same(got, want)
    assert (got[0] == 1).all() and int((got[1] > 0).sum()) > 300 and int((got[1] == 0).sum()) > 50 and got[4].max() > 500
    few = len(cs.family())
    for j, (bc, bt) in enumerate(cs.family_brute()):                                      # brute force for the n <= 12 part
        assert got[1][j] == bc and got[2][j].tolist() == bt.tolist()
    for j, k in enumerate(cs.FAN_K):                                                      # 2^k + 1 rounds to 2^k; 150 forced variables on one level
        assert got[1][few + j] == 2.0 ** k and got[4][few + j] == 2
        assert got[2][few + j][0] == got[1][few + j] and (got[2][few + j][1:] == 2.0 ** (k - 1)).all()


def test_count_positive_exactly_where_the_deciding_search_answers_one(batch):
    _, _, got, p = batch
    decided = p.exact_solve()[0].cpu().numpy()
    assert set(np.unique(decided)) == {0, 1}
    np.testing.assert_array_equal(got[1] > 0, decided == 1)
    for tc, co in zip(got[2], got[1]):
        assert (tc >= 0).all() and (tc <= co).all()


def test_marginals_agree_with_the_backbone():
    from pdp import exact
    rng = np.random.RandomState(820)
    inst = []
    while len(inst) < 8:
        n, c = cs.threshold_3sat(rng, 20, 82)
        if cm.search(n, c)[1] > 0:
            inst.append((n, c))
    items = [exact.raw_item(n, c) for n, c in inst]
    st, bb = exact.backbone(items)
    cst, count, marginals, _ = exact.count_models(items)
    assert (st == 1).all() and (cst == 1).all() and (count > 0).all()
    forced = 0
    for b, m in zip(bb, marginals):
        assert set(np.unique(b)) <= {-1, 0, 1}
        np.testing.assert_array_equal(m == 1.0, b == 1)
        np.testing.assert_array_equal(m == 0.0, b == -1)
        forced += int((b != 0).sum())
    assert forced > 10


def test_budget():
    inst = cs.family()[::5] + cs.uniform_3sat(184, 40, (3.5, 4.0, 4.6), 12)
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    full = run(inst, prob=p)
    last = None
    seen = set()
    for budget in (1, 2000, 50000):
        got = run(inst, budget, prob=p)
        st, count, tcs, work, leaves = got
        print('budget %d: complete %d of %d, count sum %g, work max %d' % (budget, int((st == 1).sum()), len(inst), count.sum(), int(work.max())))
        assert set(np.unique(st)) <= {-1, 1}
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all()
        assert (count <= full[1]).all() and (last is None or (count >= last).all())
        assert all((tc >= 0).all() and (tc <= co).all() for tc, co in zip(tcs, count))
        last = count
        seen |= set(np.unique(st))
        cs.same(got, cm.solve(inst, budget))
    assert seen == {-1, 1} and ((st == -1) & (count > 0)).any()


def test_deterministic_and_instance_local(batch, monkeypatch):
    from pdp import native
    inst, _, a, p = batch
    cs.same(a, run(inst, prob=p))                                                         # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    cs.same(cs.pick(a, order), run([inst[i] for i in order]))                             # a shuffled batch
    for i in list(range(0, len(inst), 41)) + [len(inst) - 1]:                             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            cs.same(cs.pick(a, [i]), run([inst[i]]))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every instance, one after the other
    one = run(inst, prob=p)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    cs.same(a, one)
    run(inst, prob=p)
    assert p.exact_last_grid() == len(inst)
    prev = native.use_build('fast')
    try:
        fast = run(inst)
    finally:
        native.use_build(prev)
    cs.same(a, fast)


def test_hbm_route():
    "an instance past the slab inside a batch of small ones: equal to brute force and to the model, and the same alone"
    big = cs.past_the_slab()
    few = cs.family()[:40]
    inst = few[:20] + [big] + few[20:]
    got = run(inst)
    want = cs.slab_result()
    assert (got[0][20], got[1][20], got[3][20], got[4][20]) == (want[0], want[1], want[3], want[4]) and np.array_equal(got[2][20], want[2])
    bc, bt = cs.brute(*big)
    assert got[1][20] == bc and got[2][20].tolist() == bt.tolist()
    rest = [i for i in range(len(inst)) if i != 20]
    brute = cs.family_brute()[:40]
    assert [got[1][i] for i in rest] == [b[0] for b in brute]
    assert all(got[2][i].tolist() == b[1].tolist() for i, b in zip(rest, brute))
    cs.same(cs.pick(got, [20]), run([big]))


def test_too_many_variables_in_a_batch():
    few = cs.family()[:6]
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    edge = (1023, [[1, 2], [-1, 1023]])
    inst = few[:3] + [wide] + few[3:] + [edge]
    got = run(inst)
    assert got[0].tolist() == [1, 1, 1, -2, 1, 1, 1, 1]
    assert (got[1][3], got[3][3], got[4][3]) == (0.0, 0, 0) and got[2][3].shape == (1024,) and not got[2][3].any()
    rest = [i for i in range(len(inst)) if i != 3]
    cs.same(cs.pick(got, rest), cm.solve([inst[i] for i in rest]))
    assert got[1][7] == 2.0 ** 1022 and np.isfinite(got[2][7]).all()
    alone = run([wide])
    assert (alone[0][0], alone[1][0], alone[3][0], alone[4][0]) == (-2, 0.0, 0, 0) and not alone[2][0].any()


def test_refusals(tmp_path):
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(4, 20, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_count()
    p = native.Problem(*args)
    for wrong in (1.5, '7', None, True, torch.zeros(1)):
        with pytest.raises(ValueError):
            p.exact_count(budget=wrong)
    st, count, tc, work = p.exact_count()
    assert (st.dtype, count.dtype, tc.dtype, work.dtype) == (torch.int8, torch.float64, torch.float64, torch.int64)
    assert (count.numel(), tc.numel()) == (p.B, p.V)
    status = torch.empty(p.B, dtype=torch.int8, device=p.device)
    assert native.lib().pdp_exact_count(p._h, ctypes.c_int64(0), native.ptr(status), None, None, None, None, None) != native.PDP_OK      # NULL outputs
    r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d', '--complete-count',
                        '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                       cwd=REPO)
    assert r.returncode != 0 and '--complete-count' in r.stderr and 'give --complete as well' in r.stderr


def test_count_models_segments_and_items_without_a_literal():
    from pdp import exact
    items = [exact.raw_item(3, []), exact.raw_item(2, [[], []]), exact.raw_item(4, [[]]), exact.raw_item(1024, []), exact.raw_item(1023, [])]
    st, count, marginals, work = exact.count_models(items)
    assert st.tolist() == [1, 1, 1, -2, 1] and count.tolist() == [8.0, 0.0, 0.0, 0.0, 2.0 ** 1023] and work.tolist() == [0] * 5
    assert marginals[0].tolist() == [0.5] * 3 and marginals[1] is None and marginals[2] is None and marginals[3] is None
    assert marginals[4].shape == (1023,) and (marginals[4] == 0.5).all()
    assert exact.count_is_exact(st, count).tolist() == [True, True, True, False, False]
    # through the cut along max_edges: the same answers as one problem, and brute force's
    inst = cs.family()[:60]
    raw = [exact.raw_item(n, c) for n, c in inst]
    whole, cut = exact.count_models(raw), exact.count_models(raw, max_edges=100)
    assert whole[0].dtype == np.int8 and whole[1].dtype == np.float64 and whole[3].dtype == np.int64
    for k in (0, 1, 3):
        np.testing.assert_array_equal(whole[k], cut[k])
    for a, b, (bc, bt), co in zip(whole[2], cut[2], cs.family_brute()[:60], whole[1]):
        assert co == bc and (a is None) == (b is None) == (bc == 0)
        if bc:
            assert a.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(a, bt / float(bc))


def test_cli_complete_count(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    for i in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 128)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    got, log = _run(argv + ['--complete-count', '-v'], 1, str(tmp_path / 'count.jsonl'), 0)
    assert len(base) == len(got) == 40
    new = ['model_count', 'model_count_log2', 'model_count_proved', 'marginals', 'marginal_gap', 'count_work']
    asked = proved = checked = 0
    for b, g in zip(base, got):
        r = json.loads(g)
        if r['complete'] != 1:
            assert g == b                                                                # byte-identical to the run without the flag
            continue
        assert list(r)[-6:] == new and {k: v for k, v in r.items() if k not in new} == json.loads(b)
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        st, count, tc, _, _ = cm.search(n, clauses)
        assert st == 1 and count > 0
        assert isinstance(r['model_count'], int) and r['model_count'] == int(count) and r['model_count_proved'] == 1
        # the loader keeps its own literal order, so the reads differ from the model's on the file's order; the counts cannot
        assert r['model_count_log2'] == float(np.log2(count)) and r['count_work'] > 0
        assert r['marginals'] == (tc / count).tolist()
        assert 0.0 <= r['marginal_gap'] <= 1.0
        if r['pdp_solved'] == 1:
            # PDP's prediction after Walk-SAT is its 0/1 assignment, and the check pass of the search accepted it as the row's solution
            assert r['marginal_gap'] == float(np.mean(np.abs(np.asarray(r['solution'], dtype=np.float64) - np.asarray(r['marginals']))))
            checked += 1
        asked += 1
        proved += r['model_count_proved']
    assert asked >= 5 and checked >= 3
    said = log[log.index('complete search:'):].split('\n')[0]
    assert said.endswith('; models counted for %d of %d' % (proved, asked))
