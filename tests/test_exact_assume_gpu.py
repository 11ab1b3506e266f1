"""The complete search under assumptions on the GPU (pdp_exact_solve_learn_assume): status, model, work, learned clauses, reductions and
failed sets equal to the Python statement (tests/exact_assume_model.py) on the instances of test_exact_assume_host.py -- the random
family and the constructed cases, whose statistics that file asserts -- on the LDS route, on the HBM route, in a batch of both and in
both builds of the library; A1 and A5 of the specification; instance-local outputs and no state left on the handle; the certified
answers of exact.solve_items(assume=...), exact.backbone, the --complete-backbone rows of satyr.py and the argument errors."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import exact_assume_model as am
import exact_learn_model as lm
import exact_wide as xw
import families
import test_exact_assume_host as host
from helpers import REPO
from test_exact_gpu import satisfies
from test_exact_learn_gpu import on_lds, problem, split

pytestmark = pytest.mark.gpu

PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
PAD_N = xw.LEARN_PAD_N


def flat(parts, dtype):
    return torch.from_numpy(np.concatenate([np.asarray(p, dtype=dtype) for p in parts])).to('cuda:0')


def asolve(inst, assume=None, hints=None, budget=0, arena=0, p=None):
    "(status, models, work, learned, reductions, failed index arrays) of one batch through exact_solve_assume"
    p = problem(inst) if p is None else p
    st, model, wk, failed, ln = p.exact_solve_assume(budget, hints=None if hints is None else flat(hints, np.float32),
                                                     assume=None if assume is None else flat(assume, np.int8), arena=arena, stats=True)
    red = p.exact_learn_reductions().cpu().numpy()
    return (st.cpu().numpy(), split(inst, model.cpu().numpy()), wk.cpu().numpy(), ln.cpu().numpy(), red,
            [np.nonzero(f)[0].astype(np.int64) for f in split(inst, failed.cpu().numpy())])


def same(got, want):
    "every output equal; models and failed sets of padded instances: the unpadded ones, nothing on the padding"
    for k in (0, 2, 3, 4):
        np.testing.assert_array_equal(got[k], want[k])
    for g, w in zip(got[1], want[1]):
        assert np.array_equal(g[:len(w)], w) and not g[len(w):].any()
    for g, w in zip(got[5], want[5]):
        assert np.array_equal(g, w)


def pad(inst, assume, n=PAD_N):
    """the instances over n variables, most without an occurrence: not assumed where the instance has a variable that is not, assumed false
    where every variable is assumed, so that the check pass runs for the same instances as without the padding"""
    return [(n, c) for _, c in inst], [np.concatenate([a, np.full(n - len(a), -1 if a.all() else 0, dtype=np.int8)]) for a in assume]


@functools.lru_cache(maxsize=None)
def batches():
    "arena -> (instances, assumptions, the model's six outputs): the random family with the constructed cases among it"
    inst, assume = host.random_family()
    want = host.random_results(0)[0]
    cases, res = host.constructed(), host.constructed_results()
    out = {}
    for arena in (0, host.REDUCED_ARENA):
        names = [k for k, v in cases.items() if v[2] == arena]
        if arena == 0:
            at = {k: 40 * (j + 1) for j, k in enumerate(names)}             # spread over the batch
            bi, ba, rows = list(inst), list(assume), [tuple(x[i] for x in want) for i in range(len(inst))]
            for k in names:
                bi.insert(at[k], cases[k][0]); ba.insert(at[k], cases[k][1]); rows.insert(at[k], res[k][0])
        else:
            bi, ba, rows = [cases[k][0] for k in names], [cases[k][1] for k in names], [res[k][0] for k in names]
        w = (np.array([r[0] for r in rows], dtype=np.int8), [r[1] for r in rows], np.array([r[2] for r in rows], dtype=np.int64),
             np.array([r[3] for r in rows], dtype=np.int32), np.array([r[4] for r in rows], dtype=np.int32), [r[5] for r in rows])
        out[arena] = (bi, ba, w)
    return out


def routed(route, arena):
    inst, assume, want = batches()[arena]
    if route == 'lds':
        assert all(on_lds(i, arena) for i in inst)
        return inst, assume, want
    pi, pa = pad(inst, assume)
    assert not any(on_lds(i, arena) for i in pi)
    if route == 'hbm':
        keep = [j for j in range(len(inst)) if j % 4 == 0 or len(assume[j]) > 64 or len(inst) < 10]        # every fourth, and all wide ones
        return [pi[j] for j in keep], [pa[j] for j in keep], tuple([x[j] for j in keep] if isinstance(x, list) else x[keep] for x in want)
    mix = [j % 3 == 1 for j in range(len(inst))]
    return [pi[j] if mix[j] else inst[j] for j in range(len(inst))], [pa[j] if mix[j] else assume[j] for j in range(len(inst))], want


# ---- 1. kernel = model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arena', [0, host.REDUCED_ARENA])
@pytest.mark.parametrize('route', ['lds', 'hbm', 'mixed'])
def test_equal_to_the_python_statement(route, arena):
    inst, assume, want = routed(route, arena)
    got = asolve(inst, assume, arena=arena)
    same(got, want)
    assert all(satisfies(c, m) and host.agrees(m, a) for (n, c), a, s, m in zip(inst, assume, got[0], got[1]) if s == 1)
    if arena:
        assert got[4].all()
    elif route == 'lds':
        assert (got[0] == 1).any() and any(f.size > 64 for f in got[5]) and sum(f.size == 1 for f in got[5]) > 5


def test_equal_to_the_python_statement_in_the_fast_build():
    from pdp import native
    prev = native.use_build('fast')
    try:
        for arena in (0, host.REDUCED_ARENA):
            inst, assume, want = routed('mixed', arena)
            same(asolve(inst, assume, arena=arena), want)
    finally:
        native.use_build(prev)


# ---- 2. A1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arena', [0, 40])
def test_without_assumptions_it_is_the_learning_search_on_the_same_handle(arena):
    from test_exact_learn_host import small_instances
    small = small_instances()
    family = [(n, c) for _, n, c in families.exact_cases()]
    inst = small[:90] + [lm.thrash(k) for k in (3, 7, 12)] + [family[i] for i in (9, 10, 12, 34, 35)] + [(PAD_N, c) for _, c in small[90:110]]
    p = problem(inst)
    rng = np.random.RandomState(12)
    hints = [np.where(rng.rand(n) < 0.3, np.nan, rng.randint(0, 2, size=n)).astype(np.float32) for n in xw.sizes(inst)]
    for h in (None, hints):
        ht = None if h is None else flat(h, np.float32)
        base = [t.cpu().numpy() for t in p.exact_solve(0, hints=ht, learn=True, arena=arena, stats=True)] + [p.exact_learn_reductions().cpu().numpy()]
        for a in (None, torch.zeros(p.V, dtype=torch.int8, device=p.device)):
            st, model, wk, failed, ln = p.exact_solve_assume(0, hints=ht, assume=a, arena=arena, stats=True)
            got = [st.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy(), ln.cpu().numpy(), p.exact_learn_reductions().cpu().numpy()]
            assert all(np.array_equal(x, y) for x, y in zip(got, base)) and not failed.any().item()
        if arena and h is None:
            assert base[4].any()                                         # the family instances reduce an arena of 40 words
    assert set(np.unique(base[0])) >= {0, 1}


# ---- 3. instance-local, slab-safe ----------------------------------------------------------------------------------------------------------
def test_instance_local_and_nothing_left_on_the_handle(monkeypatch):
    "many, few and no assumptions in turn, LDS and HBM routes in turn: whole, reversed, one instance per batch, one wave for all"
    inst, assume = host.random_family()
    cases = host.constructed()
    bi, ba = [], []
    for j in range(30):
        a = assume[3 * j].copy()
        if j % 3 == 1:
            a[np.nonzero(a)[0][1:]] = 0                                  # few: at most one
        if j % 3 == 2:
            a[:] = 0                                                     # none
        bi.append(inst[3 * j]); ba.append(a)
    for at, k in zip((4, 11, 18, 29), ('wide-final', 'wide-opening', 'against-level-0', 'reopened')):
        bi.insert(at, cases[k][0])
        ba.insert(at, cases[k][1])
    for j in range(0, len(bi), 5):                                       # every fifth on the HBM route
        (bi[j],), (ba[j],) = pad([bi[j]], [ba[j]])
    want = am.solve(bi, assume=ba)
    p = problem(bi)
    whole = asolve(bi, ba, p=p)
    same(whole, want)
    rev = asolve(bi[::-1], ba[::-1])
    same(tuple(x[::-1] for x in rev), want)
    for j in range(0, len(bi), 3):
        same(asolve(bi[j:j + 1], ba[j:j + 1]), tuple(x[j:j + 1] for x in want))
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    same(asolve(bi, ba, p=p), want)
    assert p.exact_last_grid() == 1
    # the learning search on the same handle, in the same slab and the same HBM arrays: no assumed or failed bit is left behind
    st, model, wk, ln = p.exact_solve(0, learn=True, stats=True)
    plain = lm.solve(bi)
    got = (st.cpu().numpy(), split(bi, model.cpu().numpy()), wk.cpu().numpy(), ln.cpu().numpy(), p.exact_learn_reductions().cpu().numpy(),
           [np.zeros(0, dtype=np.int64)] * len(bi))
    same(got, plain + ([np.zeros(0, dtype=np.int64)] * len(bi),))
    monkeypatch.delenv('PDP_EXACT_GRID')
    same(asolve(bi, ba, p=p), want)


# ---- 4. hints with assumptions ------------------------------------------------------------------------------------------------------------
def test_hints_against_assumptions_are_overridden_and_a_model_is_accepted():
    inst, assume = host.random_family()
    inst, assume = inst[:120], assume[:120]
    rng = np.random.RandomState(8)
    hints = []
    for (n, c), a in zip(inst, assume):
        h = np.where(a > 0, 0.0, 1.0).astype(np.float32)                 # against every assumption, "true first" elsewhere
        h[(rng.rand(n) < 0.3) & (a == 0)] = np.nan
        hints.append(h)
    want = am.solve(inst, hints=hints, assume=assume)
    got = asolve(inst, assume, hints=hints)
    same(got, want)
    sat = [j for j in range(len(inst)) if got[0][j] == 1]
    assert len(sat) > 20 and all(host.agrees(got[1][j], assume[j]) and satisfies(inst[j][1], got[1][j]) for j in sat)
    np.testing.assert_array_equal(got[0], am.solve(inst, assume=assume)[0])
    # A5: every variable assumed at a model's value, with hints that say the opposite
    base = am.solve(inst)
    sat = [j for j in range(len(inst)) if base[0][j] == 1]
    si = [inst[j] for j in sat]
    sa = [np.where(base[1][j] > 0.5, 1, -1).astype(np.int8) for j in sat]
    for h in (None, [1.0 - base[1][j] for j in sat]):
        got = asolve(si, sa, hints=h)
        assert (got[0] == 1).all() and not got[3].any() and all(np.array_equal(m, base[1][j]) for m, j in zip(got[1], sat))
        np.testing.assert_array_equal(got[2], [am.check_reads(inst[j][1], base[1][j])[0] for j in sat])


# ---- 5. certified answers --------------------------------------------------------------------------------------------------------------------
def test_solve_items_certifies_every_answer(monkeypatch):
    from pdp import exact, native
    inst, assume = host.random_family()
    want = host.random_results(0)[0]
    raw = [exact.raw_item(n, c, name='inst%d' % i) for i, (n, c) in enumerate(inst)]
    status, models, work, verdict, lemmas, failed = exact.solve_items(raw, assume=assume, certify=True, proofs=True, max_edges=3000)
    np.testing.assert_array_equal(status, want[0])
    np.testing.assert_array_equal(work, want[2])
    assert (verdict == 1).all()
    for j in range(len(inst)):
        assert np.array_equal(models[j], want[1][j])
        assert (failed[j] is None and lemmas[j] is None) if status[j] == 1 else (np.array_equal(failed[j], want[5][j]) and lemmas[j] is not None)
    # without certify: the same answers, and failed as the last element
    out = exact.solve_items(raw, assume=assume)
    assert len(out) == 4 and np.array_equal(out[0], status) and all(np.array_equal(x, y) for x, y in zip(out[3], failed) if x is not None)
    # a failed set that lacks a variable it needs is refuted: the CPU statement shows the instance with the rest satisfiable
    victim = drop = None
    for j in np.nonzero(want[0] == 0)[0]:
        for v in want[5][j]:
            rest = [u for u in want[5][j] if u != v]
            if len(am.brute(*am.units(inst[j][0], inst[j][1], assume[j], only=rest))) > 0:
                victim, drop = int(j), int(v)
                break
        if victim is not None:
            break
    assert victim is not None
    real = native.Problem.exact_solve_assume

    def lying(self, *a, **kw):
        out = list(real(self, *a, **kw))
        out[3][drop] = 0
        return tuple(out)

    monkeypatch.setattr(native.Problem, 'exact_solve_assume', lying)
    with pytest.raises(RuntimeError, match=r'instance 0 \(inst%d\).*satisfiable' % victim):
        exact.solve_items([raw[victim]], assume=[assume[victim]], certify=True)


def test_edge_free_instances_honour_assumptions():
    from pdp import exact
    a = np.array([1, 0, -1, 1], dtype=np.int8)
    items = [exact.raw_item(4, []), exact.raw_item(4, [[], []])]
    st, models, work, failed = exact.solve_items(items, assume=[a, a])
    assert st.tolist() == [1, 0] and models[0].tolist() == [1.0, 0.0, 0.0, 1.0] and not models[1].any()
    assert failed[0] is None and failed[1].size == 0
    st, models, work, verdict, failed = exact.solve_items(items, assume=[a, None], certify=True, hints=[np.array([0, 1, 1, 0], dtype=np.float32), None])
    assert st.tolist() == [1, 0] and models[0].tolist() == [1.0, 1.0, 0.0, 1.0] and verdict.tolist() == [1, 1]


# ---- 6. the backbone -------------------------------------------------------------------------------------------------------------------------
def test_backbone_equals_the_cpu_definition():
    from pdp import exact
    inst = host.random_family()[0][::7][:35]
    rng = np.random.RandomState(30)
    for _ in range(4):
        clauses = []
        for _ in range(120):
            vs = rng.choice(30, size=3, replace=False) + 1
            clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
        inst.append((30, clauses))
    assert len(inst) <= 40
    raw = [exact.raw_item(n, c) for n, c in inst]
    status, bbs = exact.backbone(raw)
    forced = 0
    for (n, c), s, bb in zip(inst, status, bbs):
        ws, wb = am.backbone(n, c)
        assert s == ws and ((bb is None and wb is None) or np.array_equal(bb, wb))
        forced += 0 if bb is None else int((np.abs(bb) == 1).sum())
    assert forced > 30 and (status == 1).sum() > 10 and (status == 0).sum() > 3
    # a budget of one read: nothing is decided, and nothing is claimed
    status1, bbs1 = exact.backbone(raw, budget=1)
    assert all(bb is None or set(np.unique(bb)) <= {2} for bb in bbs1) and (status1 != 0).all()
    # the base search decided, every query out of budget: code 2 only
    sat = [j for j in range(len(inst)) if status[j] == 1]
    models = exact.solve_items([raw[j] for j in sat], learn=True)[1]
    spent = exact.backbone_of([raw[j] for j in sat], np.ones(len(sat), dtype=np.int8), models, budget=1)
    assert all((bb == 2).all() for bb in spent)


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_complete_backbone(tmp_path):
    from pdp import exact
    from test_exact_trim_gpu import loader_clauses
    from test_sharded_gpu import _run
    ddir = str(tmp_path / 'cnf')
    os.makedirs(ddir)
    inst = host.random_family()[0]
    want = host.random_results(0)[0]
    for k, i in enumerate(list(range(0, 240, 20)) + [201, 203]):
        n, clauses = inst[i]
        with open(os.path.join(ddir, 'f%02d.cnf' % k), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, ddir, '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    plain, _ = _run(argv, 1, str(tmp_path / 'plain.jsonl'), 0)
    flagged, _ = _run(argv + ['--complete-backbone'], 1, str(tmp_path / 'bb.jsonl'), 0)
    a, b = [json.loads(l) for l in plain], [json.loads(l) for l in flagged]
    assert len(a) == 14 and 2 < sum(r['complete'] == 1 for r in a) < 14
    literals = 0
    for r, s in zip(a, b):
        assert list(r) == ['ID', 'label', 'solved', 'unsat_clauses', 'solution', 'complete', 'pdp_solved', 'work']        # the parent's row
        if r['complete'] == 1:
            assert list(s) == list(r) + ['backbone']
            n, clauses = loader_clauses(os.path.join(ddir, r['ID']))
            status, bbs = exact.backbone([exact.raw_item(n, clauses)])
            assert status[0] == 1 and s['backbone'] == [int(v + 1) * int(bbs[0][v]) for v in np.nonzero(bbs[0])[0]]
            assert all(s['solution'][abs(l) - 1] == (l > 0) for l in s['backbone'])
            literals += len(s['backbone'])
        else:
            assert list(s) == list(r)
        assert {k: v for k, v in s.items() if k != 'backbone'} == r
    assert literals > 10
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import satyr
    with pytest.raises(SystemExit):
        satyr.main([PDP_YAML, ddir, '100', '-d', '--complete-backbone'])


# ---- 8. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch():
    from pdp import exact
    inst = host.random_family()[0][:3]
    p = problem(inst)
    ok = torch.zeros(p.V, dtype=torch.int8, device=p.device)
    for bad in (ok.to(torch.int32), ok[:-1], ok.cpu(), [0] * p.V):
        with pytest.raises(ValueError, match='assume must be an int8 tensor'):
            p.exact_solve_assume(assume=bad)
    for arena in (-1, (1 << 30) + 1, 2.5, True):
        with pytest.raises(ValueError, match='arena'):
            p.exact_solve_assume(assume=ok, arena=arena)
    with pytest.raises(ValueError, match='hints must be a float32 tensor'):
        p.exact_solve_assume(hints=ok, assume=ok)
    assert p.exact_last_grid() == 0                                      # nothing was launched
    raw = [exact.raw_item(n, c) for n, c in inst]
    zeros = [np.zeros(n, dtype=np.int8) for n, _ in inst]
    with pytest.raises(ValueError, match='cores under assumptions'):
        exact.solve_items(raw, assume=zeros, certify=True, cores=True)
    with pytest.raises(ValueError, match='assume: one entry per instance'):
        exact.solve_items(raw, assume=zeros[:2])
    with pytest.raises(ValueError, match='assume: instance'):
        exact.solve_items(raw, assume=[zeros[0][:-1]] + zeros[1:])
    with pytest.raises(ValueError, match='assume: instance'):
        exact.solve_items(raw, assume=[zeros[0].astype(np.float32)] + zeros[1:])
    with pytest.raises(ValueError, match='arena'):
        exact.solve_items(raw, assume=zeros, arena=-1)
