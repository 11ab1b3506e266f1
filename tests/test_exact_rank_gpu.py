"""The k-th model of the counting complete search on the GPU (pdp_exact_models_at, Problem.exact_models_at, exact.models_at /
enumerate_models / sample_models, satyr.py --complete --complete-count --complete-sample): equal to its Python statement
(tests/exact_rank_model.py) bit for bit in status, count_seen, found, models, work and leaves on one problem that holds every shape the
emission can go wrong at; every row a model; the count's work and column sums; the budget; determinism over call, batch, grid and build;
the HBM route; refusals; the host layer; and the command line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_count_model as cm
import exact_rank_cases as rc
import exact_rank_model as rm
from helpers import REPO
from test_exact_count_gpu import PDP_YAML, problem

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def run(inst, ranks, budget=0, prob=None):
    "the six outputs of Problem.exact_models_at in the layout of exact_rank_model.solve"
    p = problem(inst) if prob is None else prob
    off = np.concatenate([[0], np.cumsum([len(r) for r in ranks])]).astype(np.int64)
    flat = np.asarray([int(x) for r in ranks for x in r], dtype=np.int64)
    st, seen, found, models, work, leaves = [t.cpu().numpy() for t in p.exact_models_at(torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV),
                                                                                       budget, stats=True)]
    ns = [max([n] + [abs(l) for c in cl for l in c]) for n, cl in inst]
    moff = np.concatenate([[0], np.cumsum([len(r) * n for r, n in zip(ranks, ns)])])
    assert models.shape == (moff[-1],) and found.shape == (off[-1],)
    return (st, seen, [found[off[j]:off[j + 1]] for j in range(len(inst))],
            [models[moff[j]:moff[j + 1]].reshape(len(ranks[j]), ns[j]) for j in range(len(inst))], work, leaves)


def spread(count, k=64):
    "k ranks floor(i * count / k), some of them repeated"
    r = [int(i * int(count)) // k for i in range(k)]
    return sorted(r + r[5:9])


@pytest.fixture(scope='module')
def batch():
    """A few hundred instances in one problem: the host family (n <= 12, unsatisfiable ones among them) with all ranks and one beyond,
    every seventh of them with no ranks at all; the chunk-carry shapes; the fans; uniform 3-SAT of n = 20 / 30 / 50 with spread ranks;
    the instance past the slab with its 40 ranks; an instance of 1024 variables.  The model's answers and the GPU's."""
    inst, ranks = [], []
    for j, ((n, c), r) in enumerate(zip(cs.family(), rc.family_ranks())):
        inst.append((n, c))
        ranks.append([] if j % 7 == 3 else r)
    marks = {'family': len(inst)}
    special = [(rc.fixed_prefix(), rc.PATTERNS), (rc.fixed_evens(), rc.WIDE_RANKS)] + [(cs.fan(k), [0, 5, rc.TOP]) for k in cs.FAN_K]
    special.append(((1024, [[1, 2], [-1, 1024], [3, -500, 700]]), [0, 1, 7]))
    for n, each in ((20, 8), (30, 6), (50, 2)):
        for nn, c in cs.uniform_3sat(n + 1, n, (3.5, 4.2), each):
            count = cm.search(nn, c)[1]
            special.append(((nn, c), spread(count) + [int(count)] if count < 2.0 ** 52 else spread(2 ** 52)))
    big = cs.past_the_slab()
    special.append((big, list(range(int(cs.slab_result()[1])))))
    for k, (i, r) in enumerate(special):                                                  # set between small ones
        inst += [i, cs.family()[k]]
        ranks += [r, [] if k % 2 else [0, 1]]
    marks['slab'] = marks['family'] + 2 * (len(special) - 1)
    marks['special'] = [marks['family'] + 2 * k for k in range(len(special))]
    want = rm.solve(inst, ranks)
    p = problem(inst)
    return inst, ranks, want, run(inst, ranks, prob=p), p, marks


def test_equal_to_the_python_model_exactly(batch):
    inst, ranks, want, got, _, marks = batch
    asked = sum(len(r) for r in ranks)
    print('models_at: %d instances, %d ranks, %d bytes of models, leaves max %d, work max %d'
          % (len(inst), asked, sum(m.size for m in got[3]), int(got[5].max()), int(got[4].max())))
    assert len(inst) >= 300 and asked > 10000
    rc.same(got, want)
    assert set(np.unique(got[0])) == {-2, 1}
    assert {int(v) for f in got[2] for v in f} == {-1, 0, 1}
    unsat = [j for j in range(marks['family']) if cs.family_brute()[j][0] == 0 and len(ranks[j])]
    assert len(unsat) > 30 and all(got[2][j].tolist() == [0] and got[1][j] == 0.0 for j in unsat)
    none = [j for j in range(len(inst)) if not ranks[j]]
    assert len(none) > 40 and all((got[0][j], got[1][j], got[4][j], got[5][j]) == (1, 0.0, 0, 0) for j in none)


def test_every_row_is_a_model_and_the_bits_land_in_ascending_index(batch):
    inst, ranks, _, got, _, marks = batch
    rows = 0
    for (n, c), f, m in zip(inst, got[2], got[3]):
        assert rc.satisfied(m[f == 1], c).all() and not m[f != 1].any()
        rows += int((f == 1).sum())
    assert rows > 10000
    s = marks['special']
    for r, row in zip(rc.PATTERNS, got[3][s[0]]):                                          # n = 110: the free block starts at variable 71
        assert row[:70].tolist() == [1, 0] * 35 and row[70:].tolist() == rc.bits(r, 40)
    assert got[1][s[1]] == 2.0 ** 65                                                      # n = 130: 65 free variables over three chunks
    for r, row in zip(rc.WIDE_RANKS, got[3][s[1]]):
        assert row[1::2].tolist() == [1] * 65 and row[0::2].tolist() == rc.bits(r, 53) + [0] * 12
    for j, k in zip(s[2:4], cs.FAN_K):                                                    # the fans: all three ranks in the first leaf
        assert got[5][j] == 1 and got[3][j][:, 0].tolist() == [1, 1, 1] and got[3][j][:, 1:].sum(axis=1).tolist() == [0, 2, 53]
    assert got[0][s[4]] == -2 and got[2][s[4]].tolist() == [-1, -1, -1] and got[3][s[4]].shape == (3, 1024)


def test_work_and_column_sums_against_the_count(batch):
    inst, ranks, _, got, p, marks = batch
    st, count, tc, work, leaves = [t.cpu().numpy() for t in p.exact_count(stats=True)]
    ends = np.cumsum([m.shape[1] for m in got[3]])
    tcs = np.split(tc, ends[:-1])
    beyond = full = 0
    for j, r in enumerate(ranks):
        if st[j] != 1:
            continue
        assert got[4][j] <= work[j] and got[5][j] <= leaves[j] and got[1][j] <= count[j]
        if r and r[-1] >= count[j]:
            assert (got[4][j], got[5][j], got[1][j]) == (work[j], leaves[j], count[j])
            beyond += 1
            if r == list(range(int(count[j]) + 1)):                                       # a full enumeration: the column sums are true_count
                np.testing.assert_array_equal(got[3][j][:-1].sum(axis=0, dtype=np.int64).astype(np.float64), tcs[j])
                assert len({x.tobytes() for x in got[3][j][:-1]}) == int(count[j])
                full += 1
    assert beyond > 300 and full > 300
    j = marks['slab']                                                                     # the HBM route: all 40 ranks, the brute-force models
    assert got[1][j] == count[j] == len(ranks[j]) and (got[2][j] == 1).all()
    assert {x.tobytes() for x in got[3][j]} == rc.brute_models(*inst[j])
    np.testing.assert_array_equal(got[3][j].sum(axis=0, dtype=np.int64).astype(np.float64), tcs[j])


def test_budget():
    "(c): under a smaller budget a rank is answered with the unlimited call's model or with -1"
    inst = cs.family()[::5] + cs.uniform_3sat(184, 40, (3.5, 4.0, 4.6), 6)
    ranks = [list(range(int(r[1]) + 1)) for r in rc.family_counts()[::5]] + [[0, 1000, 10 ** 6, 10 ** 9, 10 ** 12, rc.TOP]] * 18
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    full = run(inst, ranks, prob=p)
    seen = set()
    for budget in (1, 2000, 50000):
        got = run(inst, ranks, budget, prob=p)
        st, cseen, found, models, work, leaves = got
        print('budget %d: complete %d of %d, answered %d of %d ranks' % (budget, int((st == 1).sum()), len(inst), sum(int((f == 1).sum()) for f in found),
                                                                         sum(len(r) for r in ranks)))
        assert set(np.unique(st)) <= {-1, 1}
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all() and (work <= full[4]).all() and (cseen <= full[1]).all()
        for j in range(len(inst)):
            a = found[j] == 1
            np.testing.assert_array_equal(models[j][a], full[3][j][a])
            assert not models[j][~a].any() and ((found[j] == full[2][j]) | (found[j] == -1)).all()
            assert (st[j] == -1) == bool((found[j] == -1).any())
        seen |= set(np.unique(st))
        rc.same(got, rm.solve(inst, ranks, budget))
    assert seen == {-1, 1}


def test_deterministic_and_instance_local(batch, monkeypatch):
    from pdp import native
    inst, ranks, _, a, p, marks = batch
    rc.same(a, run(inst, ranks, prob=p))                                                  # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    rc.same(rc.pick(a, order), run([inst[i] for i in order], [ranks[i] for i in order]))  # a shuffled batch
    for i in list(range(0, len(inst), 61)) + marks['special'][:4] + [marks['slab']]:      # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            rc.same(rc.pick(a, [i]), run([inst[i]], [ranks[i]]))
    i = max(j for j in range(marks['family']) if len(ranks[j]) > 6 and inst[j][1])         # the answer to a rank does not depend on the others
    some = ranks[i][::3]
    alone = run([inst[i]], [some])
    np.testing.assert_array_equal(alone[3][0], a[3][i][::3])
    monkeypatch.setenv('PDP_EXACT_GRID', '1')                                             # one wave takes every instance, one after the other
    one = run(inst, ranks, prob=p)
    assert p.exact_last_grid() == 1
    monkeypatch.delenv('PDP_EXACT_GRID')
    rc.same(a, one)
    run(inst, ranks, prob=p)
    assert p.exact_last_grid() == len(inst)
    prev = native.use_build('fast')
    try:
        fast = run(inst, ranks)
    finally:
        native.use_build(prev)
    rc.same(a, fast)


def test_refusals():
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(4, 20, 3, seed=1)), torch.device(DEV))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=DEV)
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_models_at(t([]), torch.zeros(p.B + 1, dtype=torch.int64, device=DEV))
    p = native.Problem(*args)
    good = p.exact_models_at(t([0, 1, 2]), t([0, 2, 2, 3, 3]))
    assert [x.dtype for x in good] == [torch.int8, torch.float64, torch.int8, torch.uint8, torch.int64]
    assert [x.numel() for x in good] == [4, 4, 3, 60, 4]
    for ranks, off, says in (([1, 0], [0, 2, 2, 2, 2], 'ranks of instance 0 decrease'), ([0, 0, 5, 4], [0, 1, 2, 4, 4], 'ranks of instance 2 decrease'),
                             ([0, 1 << 53], [0, 1, 1, 1, 2], 'rank of instance 3 is not in'), ([-1], [0, 0, 1, 1, 1], 'rank of instance 1 is not in'),
                             ([0, 1], [1, 1, 2, 2, 2], 'does not start at 0'), ([0, 1], [0, 2, 1, 2, 2], 'rank_off decreases at instance 1')):
        with pytest.raises(native.NativeError, match='error 1.*' + says):
            p.exact_models_at(t(ranks), t(off))
    for ranks, off in ((t([0]).to(torch.int32), t([0, 1, 1, 1, 1])), (t([0]), t([0, 1, 1, 1])), (t([0, 1]), t([0, 1, 1, 1, 1])),
                       (t([0]).cpu(), t([0, 1, 1, 1, 1])), ([0], t([0, 1, 1, 1, 1])), (t([0]), t([0, 1, 1, 1, 1]).to(torch.int32))):
        with pytest.raises(ValueError):
            p.exact_models_at(ranks, off)
    for wrong in (1.5, '7', None, True):
        with pytest.raises(ValueError):
            p.exact_models_at(t([0]), t([0, 1, 1, 1, 1]), budget=wrong)
    rc_ = [x.cpu().numpy() for x in p.exact_models_at(t([0, 1, 2]), t([0, 2, 2, 3, 3]))]  # the handle still answers, and the same
    for x, y in zip(good, rc_):
        np.testing.assert_array_equal(x.cpu().numpy(), y)


def test_models_at_segments_unsorted_input_and_items_without_a_literal():
    from pdp import exact
    items = [exact.raw_item(3, []), exact.raw_item(2, [[], []]), exact.raw_item(1024, []), exact.raw_item(70, []), exact.raw_item(4, [])]
    st, seen, found, models, work = exact.models_at(items, [[5, 0, 8, 7], [0], [1], [rc.TOP, 3], None])
    assert st.tolist() == [1, 1, -2, 1, 1] and seen.tolist() == [8.0, 0.0, 0.0, 2.0 ** 70, 0.0] and work.tolist() == [0] * 5
    assert found[0].tolist() == [1, 1, 0, 1] and models[0].tolist() == [[1, 0, 1], [0, 0, 0], [0, 0, 0], [1, 1, 1]]
    assert found[1].tolist() == [0] and found[2].tolist() == [-1] and models[2].shape == (1, 1024)
    assert models[3][0].tolist() == [1] * 53 + [0] * 17 and models[3][1].tolist() == [1, 1] + [0] * 68
    assert found[4].shape == (0,) and models[4].shape == (0, 4) and models[4].dtype == np.uint8
    # through the cut along max_edges, in the caller's order: the same answers as one sorted problem
    inst, all_ranks = cs.family()[:60], rc.family_ranks()[:60]
    raw = [exact.raw_item(n, c) for n, c in inst]
    rng = np.random.RandomState(3)
    perm = [rng.permutation(len(r)) for r in all_ranks]
    asked = [np.asarray(r, dtype=np.int64)[q] for r, q in zip(all_ranks, perm)]
    asked[7] = None
    whole, cut = exact.models_at(raw, asked), exact.models_at(raw, asked, max_edges=100)
    want = rm.solve(inst, [r if k != 7 else [] for k, r in enumerate(all_ranks)])
    for k in (0, 1, 4):
        np.testing.assert_array_equal(whole[k], want[k])
        np.testing.assert_array_equal(cut[k], want[k])
    for j, q in enumerate(perm):
        for res in (whole, cut):
            if j == 7:
                assert res[2][j].shape == (0,) and res[3][j].shape == (0, want[3][j].shape[1])
            else:
                assert res[3][j].dtype == np.uint8 and np.array_equal(res[2][j], want[2][j][q]) and np.array_equal(res[3][j], want[3][j][q])
    with pytest.raises(ValueError):
        exact.models_at(raw[:2], [[0], [1 << 53]])
    with pytest.raises(ValueError):
        exact.models_at(raw[:2], [[0]])


def test_enumerate_models():
    from pdp import exact
    inst = cs.family()[:50] + [(3, []), (2, [[]])]
    raw = [exact.raw_item(n, c) for n, c in inst]
    models, complete = exact.enumerate_models(raw, 20)
    counts = [b[0] for b in cs.family_brute()[:50]] + [8, 0]
    assert any(c > 20 for c in counts) and any(c == 0 for c in counts) and any(0 < c <= 20 for c in counts)
    for (n, c), m, done, bc in zip(inst, models, complete, counts):
        assert m.dtype == np.uint8 and m.shape[0] == min(bc, 20) and bool(done) == (bc <= 20)
        rows = {r.tobytes() for r in m}
        assert len(rows) == m.shape[0] and rows <= rc.brute_models(n, c) and (not done or len(rows) == bc)


def test_sample_models_against_models_at():
    from pdp import exact
    inst = cs.uniform_3sat(77, 24, (3.0, 4.0), 4) + [cs.fan(60), (2, [[1], [-1]]), (1024, [[1, 2]]), (5, [])]
    raw = [exact.raw_item(n, c) for n, c in inst]
    counts = exact.count_models(raw)
    samples, ranks = exact.sample_models(raw, 32, seed=11, counts=counts)
    ok = exact.count_is_exact(counts[0], counts[1]) & (counts[1] > 0)
    assert ok.tolist()[-4:] == [False, False, False, True] and ok[:8].sum() >= 4          # 2^60 + 1 rounds: above 2^53; no model; too wide
    asked = [r if r is not None else [] for r in ranks]
    at = exact.models_at(raw, asked)
    for i, ((n, c), s, r) in enumerate(zip(inst, samples, ranks)):
        assert (s is None) == (r is None) == (not ok[i])
        if ok[i]:
            np.testing.assert_array_equal(r, exact.sample_ranks(counts[1][i], 32, 11, i))
            assert s.shape == (32, n) and np.array_equal(s, at[3][i]) and rc.satisfied(s, c).all()
    again, _ = exact.sample_models(raw, 32, seed=11)                                      # runs count_models itself: the same draw
    other, _ = exact.sample_models(raw, 32, seed=12, counts=counts)
    assert all((a is None and s is None) or np.array_equal(a, s) for a, s in zip(again, samples))
    assert any(s is not None and not np.array_equal(o, s) for o, s in zip(other, samples))
    # an instance's draw does not depend on its batch, only on its index
    solo, _ = exact.sample_models(raw[:1], 32, seed=11)
    np.testing.assert_array_equal(solo[0], samples[0])


def test_cli_complete_sample(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    import satyr
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
    got, log = _run(argv + ['--complete-sample', '5', '-v'], 1, str(tmp_path / 'sample.jsonl'), 0)
    assert len(base) == len(got) == 40
    sampled = asked = 0
    for b, g in zip(base, got):
        r = json.loads(g)
        if 'samples' not in r:
            assert g == b                                                                 # byte-identical to the run without the flag
            asked += r['complete'] == 1
            continue
        assert list(r)[-2:] == ['samples', 'sample_ranks'] and {k: v for k, v in r.items() if k not in ('samples', 'sample_ranks')} == json.loads(b)
        assert r['model_count_proved'] == 1 and isinstance(r['model_count'], int) and r['model_count'] > 0
        n, clauses = dimacs2json.parse_dimacs(str(ddir / r['ID']))
        s = np.asarray(r['samples'])
        assert s.shape == (5, n) and len(r['solution']) == n and set(np.unique(s)) <= {0, 1} and rc.satisfied(s, clauses).all()
        assert len(r['sample_ranks']) == 5 and all(isinstance(x, int) and 0 <= x < r['model_count'] for x in r['sample_ranks'])
        sampled += 1
        asked += 1
    assert sampled >= 5
    said = log[log.index('complete search:'):].split('\n')[0]
    assert said.endswith('; sampled %d of %d' % (sampled, asked))
    for bad in (['--complete', '--complete-sample', '3'], ['--complete', '--complete-count', '--complete-sample', '0']):
        with pytest.raises(SystemExit):
            satyr.main([PDP_YAML, str(ddir), '10', '-d'] + bad)
