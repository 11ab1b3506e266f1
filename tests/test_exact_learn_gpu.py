"""The learning complete search on the GPU (pdp_exact_solve_learn, Problem.exact_solve(learn=True), exact.solve_items(learn=True),
satyr.py --complete --complete-learn): equal to its Python statement (tests/exact_learn_model.py) in status, model, work and learned
clauses on both routes and at arenas that are reduced and exhausted; the family chronological backtracking cannot handle; agreement
with pdp_exact_solve; determinism, hints, budget, refusals and the command line."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import exact_learn_model as lm
import exact_model
import families
from helpers import REPO
from test_exact_gpu import planted, satisfies
from test_exact_learn_host import edges, small_instances

pytestmark = pytest.mark.gpu

PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
PAD_N = 1400                 # variables (most without an occurrence) that put any instance on the HBM route: 37 bytes of slab each


def slab_bytes(n, m, e, arena):
    "exl_lds_layout of csrc/pdp_exact.hip: an instance takes the LDS route up to 48 KiB, with e + A <= 65535"
    A = arena if arena else 4 * e
    return (37 * n + 4 + 2 * (e + A) + 2 * (m + 1) + 15) & ~15


def on_lds(inst, arena):
    n, c = inst
    e = sum(len(x) for x in c)
    n = max([n] + [abs(l) for x in c for l in x])
    return slab_bytes(n, len(c), e, arena) <= 48 * 1024 and e + (arena if arena else 4 * e) <= 65535


def problem(inst):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment([exact.raw_item(n, c) for n, c in inst]), torch.device('cuda:0'))
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(inst))


def split(inst, model):
    sizes = [max([n] + [abs(l) for x in c for l in x]) for n, c in inst]
    return [m.copy() for m in np.split(model, np.cumsum(sizes)[:-1])]


def lsolve(inst, hints=None, budget=0, arena=0, learn=True):
    "(status, models, work, learned, reductions) of one batch; learn=False: pdp_exact_solve(_hinted) with None for the last two"
    p = problem(inst)
    hint = None if hints is None else torch.from_numpy(np.concatenate([np.asarray(h, dtype=np.float32) for h in hints])).to(p.device)
    if learn:
        st, model, wk, ln = p.exact_solve(budget, hints=hint, learn=True, arena=arena, stats=True)
        ln, red = ln.cpu().numpy(), p.exact_learn_reductions().cpu().numpy()
    else:
        (st, model, wk), ln, red = p.exact_solve(budget, hints=hint), None, None
    return st.cpu().numpy(), split(inst, model.cpu().numpy()), wk.cpu().numpy(), ln, red


def same(a, b):
    "status, work, learned, reductions (where both sides have them) and every model equal"
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])
    if len(a) > 4 and len(b) > 4:
        np.testing.assert_array_equal(a[4], b[4])
    assert all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))


def thrashes():
    return [lm.thrash(k) for k in range(2, 13)]


def family():
    return [(n, c) for _, n, c in families.exact_cases()]


@pytest.fixture(scope='module')
def inputs():
    "the small instances of the host test, families.exact_cases() and thrash k = 2 .. 12, with the model's results at the three arenas"
    inst = small_instances() + family() + thrashes()
    return inst, {A: lm.solve(inst, arena=A) for A in (0, 12, 40)}


@pytest.mark.parametrize('arena', [0, 12, 40])
def test_equal_to_the_python_model_on_the_lds_route(inputs, arena):
    inst, want = inputs
    assert all(on_lds(i, arena) for i in inst)
    got = lsolve(inst, arena=arena)
    same(got, want[arena])
    if arena:
        assert got[4].any() and (arena == 40 or (got[0] == -1).any())                # 40 words are reduced, 12 words also run out
    assert all(satisfies(c, m) for (n, c), s, m in zip(inst, got[0], got[1]) if s == 1)


@pytest.mark.parametrize('arena', [0, 12, 40])
def test_equal_to_the_python_model_on_the_hbm_route(inputs, arena):
    "the same clauses over PAD_N variables: the slab is past 48 KiB, the arena is an HBM block; the outputs are the unpadded ones"
    inst, want = inputs
    keep = list(range(0, 420, 5)) + list(range(420, len(inst)))
    padded = [(PAD_N, inst[i][1]) for i in keep]
    assert not any(on_lds(i, arena) for i in padded)
    st, models, wk, ln, red = lsolve(padded, arena=arena)
    w = want[arena]
    np.testing.assert_array_equal(st, w[0][keep])
    np.testing.assert_array_equal(wk, w[2][keep])
    np.testing.assert_array_equal(ln, w[3][keep])
    np.testing.assert_array_equal(red, w[4][keep])
    assert red.any() == (arena != 0)
    for j, i in enumerate(keep):
        k = len(w[1][i])
        assert np.array_equal(models[j][:k], w[1][i]) and not models[j][k:].any()


def test_thrash_is_decided_where_backtracking_runs_out_of_budget():
    "k = 12, n = 27: chronological backtracking needs over 2 000 000 reads (host test); learning needs the model's 1 742"
    n, clauses = lm.thrash(12)
    assert n == 27
    plain = lsolve([(n, clauses)], budget=200_000, learn=False)
    assert plain[0].tolist() == [-1]
    st, models, wk, ln, _ = lsolve([(n, clauses)], budget=200_000)
    want = lm.search(n, clauses, budget=200_000)
    assert st.tolist() == [0] and wk.tolist() == [want[2]] and ln.tolist() == [want[3]] and wk[0] < 10_000 and not models[0].any()


def threshold(count, n=50, seed=77):
    rng = np.random.RandomState(seed)
    inst = []
    for _ in range(count):
        clauses = []
        for _ in range(int(round(4.26 * n))):
            vs = rng.choice(n, size=3, replace=False) + 1
            clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
        inst.append((n, clauses))
    return inst


def test_status_agrees_with_pdp_exact_solve():
    """64 threshold instances at n = 50: at the default arena (LDS route, reduced now and then), at 20 000 words (LDS route) and at 40 000
    words (the slab is past 48 KiB: HBM arena).  No clause has more than n literals, so an arena of 20 000 words cannot fill while
    learned * (n + 1) stays below it: the two large arenas then give one search, on two routes."""
    inst = threshold(64)
    plain = lsolve(inst, learn=False)
    assert set(np.unique(plain[0])) == {0, 1}
    assert all(on_lds(i, 0) and on_lds(i, 20000) and not on_lds(i, 40000) for i in inst)
    runs = {A: lsolve(inst, arena=A) for A in (0, 20000, 40000)}
    for A, got in runs.items():
        np.testing.assert_array_equal(got[0], plain[0])
        assert all(satisfies(c, m) if s == 1 else not m.any() for (n, c), s, m in zip(inst, got[0], got[1]))
    assert runs[20000][3].max() * 51 <= 20000
    same(runs[20000], runs[40000])


def test_status_agrees_on_composed_instances_on_the_hbm_route():
    "threshold cores (both answers) first, last and interleaved in a planted instance of 1 000 variables, among small instances"
    big = planted(1000, 2.0, 3, 10)
    cores = families.threshold_cores()
    inst = [families.compose(core, big, place)[:2] for place in ('first', 'last', 'interleaved') for core in cores]
    mixed = threshold(3) + inst[:6] + thrashes()[:4] + inst[6:]
    assert not any(on_lds(i, 0) for i in inst) and not any(on_lds(i, 40) for i in inst)
    plain = lsolve(mixed, learn=False)
    assert {0, 1} <= set(np.unique(plain[0][3:9]))
    for arena in (0, 40):
        got = lsolve(mixed, arena=arena)
        decided = got[0] != -1
        assert decided.all() or arena == 40
        np.testing.assert_array_equal(got[0][decided], plain[0][decided])
        assert all(satisfies(c, m) if s == 1 else not m.any() for (n, c), s, m in zip(mixed, got[0], got[1]))


def modular(count=8):
    "the reference's community-attachment family (pdp.cnf_generators, which draws from numpy's global generator: seeded and restored)"
    from pdp.cnf_generators import ModularCNFGenerator
    saved = np.random.get_state()
    np.random.seed(3)
    try:
        g = ModularCNFGenerator(3, 60, 60, 0.8, 0.9, 6, 6, 4.0, 4.4, 1)
        out = []
        for _ in range(count):
            r = g.generate_complete()
            out.append((int(r[0]), [[int(l) for l in c] for c in r[6]]))
    finally:
        np.random.set_state(saved)
    return out


def test_modular_family():
    inst = modular()
    got = lsolve(inst)
    same(got, lm.solve(inst))
    plain = lsolve(inst, learn=False)
    np.testing.assert_array_equal(got[0], plain[0])
    assert set(np.unique(got[0])) <= {0, 1}
    print("modular n = 60: learning %d reads, backtracking %d reads" % (got[2].sum(), plain[2].sum()))
    assert got[2].sum() < plain[2].sum()


def test_deterministic_and_instance_local(inputs):
    from pdp import native
    inst, want = inputs
    probe = int(np.argmax(want[0][3]))                                # the instance that learns the most clauses
    few = [inst[i] for i in range(0, 420, 9)]
    for arena in (0, 40):
        w = want[arena]
        one = tuple(x[probe:probe + 1] for x in w)
        p = problem([inst[probe]])
        a = [t.cpu().numpy() for t in p.exact_solve(learn=True, arena=arena, stats=True)]
        b = [t.cpu().numpy() for t in p.exact_solve(learn=True, arena=arena, stats=True)]      # the same problem called twice
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0][0] == one[0][0] and a[2][0] == one[2][0] and a[3][0] == one[3][0]
        for batch, at in (([inst[probe]] + few, 0), (few + [inst[probe]], len(few)), (few[:20] + [inst[probe]] + few[20:], 20)):
            got = lsolve(batch, arena=arena)
            same(tuple(x[at:at + 1] for x in got), one)
    assert want[0][3][probe] > 10
    prev = native.use_build('fast')
    try:
        fast = {A: lsolve(inst, arena=A) for A in (0, 40)}
    finally:
        native.use_build(prev)
    for A in (0, 40):
        same(fast[A], want[A])


def test_hints(inputs):
    from pdp import native
    inst, want = inputs
    rng = np.random.RandomState(8)
    base = want[0]
    # no hints: a NULL pointer, hints=None and an all-NaN tensor
    p = problem(inst)
    status = torch.empty(p.B, dtype=torch.int8, device=p.device)
    model = torch.empty(p.V, dtype=torch.float32, device=p.device)
    work = torch.empty(p.B, dtype=torch.int64, device=p.device)
    learned = torch.empty(p.B, dtype=torch.int32, device=p.device)
    native.check(native.lib().pdp_exact_solve_learn(p._h, ctypes.c_void_p(0), ctypes.c_int64(0), ctypes.c_int64(0), native.ptr(status),
                                                    native.ptr(model), native.ptr(work), native.ptr(learned), native._stream()))
    nan = torch.full((p.V,), float('nan'), dtype=torch.float32, device=p.device)
    for got in ((status, model, work, learned), p.exact_solve(learn=True, stats=True), p.exact_solve(hints=nan, learn=True, stats=True)):
        st, mo, wk, ln = [t.cpu().numpy() for t in got]
        same((st, split(inst, mo), wk, ln), base)
    # the work pointer and the learned pointer may be NULL
    native.check(native.lib().pdp_exact_solve_learn(p._h, ctypes.c_void_p(0), ctypes.c_int64(0), ctypes.c_int64(0), native.ptr(status),
                                                    native.ptr(model), ctypes.c_void_p(0), ctypes.c_void_p(0), native._stream()))
    np.testing.assert_array_equal(status.cpu().numpy(), base[0])
    # the run's own model: the check pass accepts it, work = its reads
    hints = [m.copy() for m in base[1]]
    own = lsolve(inst, hints=hints)
    same(own, lm.solve(inst, hints=hints))
    sat = base[0] == 1
    reads = np.array([exact_model.check_reads(c, m)[0] for (_, c), m in zip(inst, base[1])], dtype=np.int64)
    np.testing.assert_array_equal(own[0][sat], base[0][sat])
    np.testing.assert_array_equal(own[2][sat], reads[sat])
    assert not own[3][sat].any() and all(np.array_equal(a, b) for a, b, s_ in zip(own[1], base[1], sat) if s_)
    # random phases with 30 % NaN, and complete random assignments: the model's polarity rule and check pass
    for frac in (0.3, 0.0):
        hints = []
        for m in base[1]:
            h = rng.randint(0, 2, size=len(m)).astype(np.float32)
            h[rng.rand(len(m)) < frac] = np.nan
            hints.append(h)
        for arena in (0, 40):
            same(lsolve(inst, hints=hints, arena=arena), lm.solve(inst, hints=hints, arena=arena))


def test_budget():
    "budgets 1, e and 10 e on five threshold instances of one size (n = 60, e = 768): the bound, and a decided status is the unbounded one"
    inst = [(n, c) for name, n, c in families.exact_cases() if name.startswith('ladder-n60')]
    e = edges(inst)
    assert len(inst) == 5 and (e == e[0]).all()
    for arena in (0, 40):
        A = arena if arena else 4 * e
        full = lsolve(inst, arena=arena)
        for budget in (1, int(e[0]), 10 * int(e[0])):
            got = lsolve(inst, budget=budget, arena=arena)
            same(got, lm.solve(inst, budget=budget, arena=arena))
            assert (got[2] < budget + 4 * (e + A)).all()
            done = got[0] != -1
            np.testing.assert_array_equal(got[0][done], full[0][done])
            np.testing.assert_array_equal(got[2][done], full[2][done])
        assert (lsolve(inst, budget=1, arena=arena)[0] == -1).all()


def test_refusals():
    from pdp import exact, native
    from pdp.factorgraph import dataset
    items = dataset.random_ksat_items(4, 20, 3, seed=1)
    b = dataset.to_torch(dataset.collate_segment(items), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_solve(learn=True)
    p = native.Problem(*args)
    with pytest.raises(native.NativeError, match='error 1'):
        p.exact_learn_reductions()                                    # no learning call on this problem yet
    for kw in (dict(learn=True, arena=-1), dict(learn=True, arena=(1 << 30) + 1), dict(learn=True, arena=2.5), dict(arena=40), dict(stats=True),
               dict(learn=True, hints=torch.zeros(p.V + 1, dtype=torch.float32, device=p.device))):
        with pytest.raises(ValueError):
            p.exact_solve(**kw)
    with pytest.raises(ValueError):
        exact.solve_items(items, arena=40)
    status, models, work = exact.solve_items(items, learn=True, arena=40)
    np.testing.assert_array_equal(status, exact.solve_items(items)[0])
    assert exact.label_clause_lists([lm.thrash(12)], budget=200_000) == [None]
    assert exact.label_clause_lists([lm.thrash(12)], budget=200_000, learn=True) == [False]
    assert exact.is_sat(3, [[1, 2], [-1, 3]], learn=True) is True


def test_cli_complete_learn(tmp_path):
    from test_sharded_gpu import _run
    ddir = os.path.join(REPO, 'tests', 'golden', 'dimacs20')
    argv = [PDP_YAML, ddir, '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    plain, _ = _run(argv, 1, str(tmp_path / 'plain.jsonl'), 0)
    learn, _ = _run(argv + ['--complete-learn'], 1, str(tmp_path / 'learn.jsonl'), 0)
    a, b = [json.loads(l) for l in plain], [json.loads(l) for l in learn]
    assert len(a) == 20 and [r['ID'] for r in a] == [r['ID'] for r in b]
    assert [list(r) for r in a] == [list(r) for r in b]
    assert [r['complete'] for r in a] == [r['complete'] for r in b] and {r['complete'] for r in a} <= {0, 1}
    assert [r['pdp_solved'] for r in a] == [r['pdp_solved'] for r in b]
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    for r in b:
        if r['complete'] == 1:
            assert satisfies(dimacs2json.parse_dimacs(os.path.join(ddir, r['ID']))[1], r['solution'])
