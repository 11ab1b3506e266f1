"""Proof logging and proof checking on the GPU (pdp_exact_solve_learn_proof, pdp_exact_check; Problem.exact_solve_proof / exact_check,
exact.solve_items(certify=True), satyr.py --complete --complete-certify, dimacs2json.py --label exact-certified): equal to their Python
statements (tests/exact_proof_model.py) word for word and read for read on both routes of both kernels; the regions and what is left
untouched; mutated, forged and malformed proofs; wide lemmas and long proofs; the checker's budget; determinism; hints; refusals; the
command line."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import exact_learn_model as lm
import exact_model
import exact_proof_model as pm
import exact_wide
import families
from helpers import REPO
from test_exact_learn_gpu import PAD_N, PDP_YAML, on_lds, problem, split

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
CHECK_PAD_N = 10000          # the checker's slab takes 5 bytes per variable (request word, value byte): 10 000 variables are past 48 KiB


def check_on_lds(inst):
    "exc_lds_layout of csrc/pdp_exact.hip: 4 n + 2 e + 2 (m + 1) + n bytes, up to 48 KiB"
    n, c = inst
    e = sum(len(x) for x in c)
    n = max([n] + [abs(l) for x in c for l in x])
    return ((5 * n + 2 * e + 2 * (len(c) + 1) + 15) & ~15) <= 48 * 1024 and e <= 65535


def run_proof(inst, hints=None, budget=0, arena=0, sizes=None, prob=None):
    """one call of exact_solve_proof on a sentinel-filled buffer: dict of numpy outputs; ``sizes``: region words per instance (None: the
    default regions); 'words' = per instance the first min(proof_len, size) words of its region"""
    p = problem(inst) if prob is None else prob
    hint = None if hints is None else torch.from_numpy(np.concatenate([np.asarray(h, dtype=np.float32) for h in hints])).to(p.device)
    off = None
    if sizes is not None:
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(p.device)
        total = int(np.sum(sizes))
    else:
        from pdp import native
        total = int(p.instance_edges().sum().item()) * native.PROOF_WORDS_PER_LITERAL
    buf = torch.full((total + 7,), SENTINEL, dtype=torch.int32, device=p.device)
    st, model, wk, ln, proof, off, plen = p.exact_solve_proof(budget, hints=hint, arena=arena, proof_off=off, proof=buf)
    red = p.exact_learn_reductions().cpu().numpy()
    out = dict(status=st.cpu().numpy(), models=split(inst, model.cpu().numpy()), work=wk.cpu().numpy(), learned=ln.cpu().numpy(), reductions=red,
               proof=proof.cpu().numpy(), off=off.cpu().numpy(), plen=plen.cpu().numpy(), prob=p)
    size = out['off'][1:] - out['off'][:-1]
    out['size'] = size
    out['words'] = [out['proof'][a:a + min(k, s)] for a, k, s in zip(out['off'][:-1], out['plen'], size)]
    return out


def untouched(out):
    "every word outside the stored lemmas still holds the sentinel"
    mask = np.ones(len(out['proof']), dtype=bool)
    for a, w in zip(out['off'][:-1], out['words']):
        mask[a:a + len(w)] = False
    return bool((out['proof'][mask] == SENTINEL).all())


def run_check(inst, status, models, regions, plen, budget=0, prob=None):
    "one call of exact_check: numpy (verdict, fail_at, work); ``regions``: the int32 words of every instance's region"
    p = problem(inst) if prob is None else prob
    sizes = exact_wide.sizes(inst)
    model = np.concatenate([np.concatenate([np.asarray(m, dtype=np.float32), np.zeros(n - len(m), dtype=np.float32)]) for m, n in zip(models, sizes)])
    off = np.concatenate([[0], np.cumsum([len(r) for r in regions])]).astype(np.int64)
    proof = np.concatenate([np.asarray(r, dtype=np.int32) for r in regions] + [np.full(3, SENTINEL, dtype=np.int32)])
    dev = p.device
    out = p.exact_check(torch.from_numpy(np.asarray(status, dtype=np.int8)).to(dev), torch.from_numpy(model).to(dev), torch.from_numpy(proof).to(dev),
                        torch.from_numpy(off).to(dev), torch.from_numpy(np.asarray(plen, dtype=np.int64)).to(dev), budget)
    return tuple(t.cpu().numpy() for t in out)


def same_check(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def same_search(out, want):
    "status, models, work, learned, reductions, lemma words and proof_len equal to pm.solve's"
    np.testing.assert_array_equal(out['status'], want[0])
    np.testing.assert_array_equal(out['work'], want[2])
    np.testing.assert_array_equal(out['learned'], want[3])
    np.testing.assert_array_equal(out['reductions'], want[4])
    np.testing.assert_array_equal(out['plen'], want[6])
    for got, m, lemmas in zip(out['models'], want[1], want[5]):
        assert np.array_equal(got[:len(m)], m) and not got[len(m):].any()
    for got, lemmas, size in zip(out['words'], want[5], out['size']):
        stored = pm.region(lemmas, size)                                             # whole lemmas only; what follows them is not touched
        np.testing.assert_array_equal(got[:len(stored)], stored)
        assert (got[len(stored):] == SENTINEL).all()


def take(want, keep):
    return tuple([w[i] for i in keep] if isinstance(w, list) else w[keep] for w in want)


# ---- 1. logging ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arena', [0, 12, 40])
def test_logging_equals_the_python_model_on_the_lds_route(arena):
    inst, want = pm.base_inputs()
    assert all(on_lds(i, arena) for i in inst)
    out = run_proof(inst, arena=arena)
    same_search(out, want[arena])
    assert (out['plen'] <= out['size']).all() and out['plen'].max() > 30 and untouched(out)
    # the other outputs are pdp_exact_solve_learn's on the same problem
    p = out['prob']
    st, model, wk, ln = [t.cpu().numpy() for t in p.exact_solve(learn=True, arena=arena, stats=True)]
    np.testing.assert_array_equal(st, out['status'])
    np.testing.assert_array_equal(wk, out['work'])
    np.testing.assert_array_equal(ln, out['learned'])
    np.testing.assert_array_equal(p.exact_learn_reductions().cpu().numpy(), out['reductions'])
    assert all(np.array_equal(a, b) for a, b in zip(split(inst, model), out['models']))


@pytest.mark.parametrize('arena', [0, 12, 40])
def test_logging_equals_the_python_model_on_the_hbm_route(arena):
    inst, want = pm.base_inputs()
    keep = list(range(0, 420, 5)) + list(range(420, len(inst)))
    padded = [(PAD_N, inst[i][1]) for i in keep]
    assert not any(on_lds(i, arena) for i in padded)
    out = run_proof(padded, arena=arena)
    same_search(out, take(want[arena], keep))
    assert untouched(out) and out['plen'].max() > 30
    p = out['prob']
    st, model, wk, ln = [t.cpu().numpy() for t in p.exact_solve(learn=True, arena=arena, stats=True)]
    assert np.array_equal(st, out['status']) and np.array_equal(wk, out['work']) and np.array_equal(ln, out['learned'])
    np.testing.assert_array_equal(p.exact_learn_reductions().cpu().numpy(), out['reductions'])


# ---- 2. regions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [0, PAD_N])
def test_regions(pad):
    inst, want = pm.base_inputs()
    keep = list(range(len(inst))) if not pad else list(range(0, 420, 5)) + list(range(420, len(inst)))
    batch = [(max(pad, inst[i][0]), inst[i][1]) for i in keep]
    w = take(want[0], keep)
    full = run_proof(batch)
    same_search(full, w)
    sizes = full['size'].copy()
    cut = np.arange(len(batch)) % 3 == 0
    sizes[cut] = full['plen'][cut] // 2
    out = run_proof(batch, sizes=sizes)
    same_search(out, w)                                                              # the search does not depend on the regions
    assert untouched(out)
    short = cut & (full['plen'] > 0)
    assert short.sum() > 10 and (out['plen'][short] > out['size'][short]).all()
    stored = 0
    for b in range(len(batch)):
        if cut[b]:
            k = len(pm.region(w[5][b], sizes[b]))
            np.testing.assert_array_equal(out['proof'][out['off'][b]:out['off'][b] + k], full['words'][b][:k])
            assert (out['proof'][out['off'][b] + k:out['off'][b + 1]] == SENTINEL).all()
            stored += k > 0
        else:
            np.testing.assert_array_equal(out['words'][b], full['words'][b])
    assert stored > 5                                                                # prefixes that are neither empty nor whole
    # the sizing call: no buffer, regions of no words
    p = out['prob']
    r = p.exact_solve_proof(proof_off=torch.zeros(p.B + 1, dtype=torch.int64, device=p.device))
    assert r[4] is None
    np.testing.assert_array_equal(r[6].cpu().numpy(), full['plen'])
    np.testing.assert_array_equal(r[0].cpu().numpy(), full['status'])


# ---- 3. the checker --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def check_cases(pad):
    """(instances, status, models, regions, proof_len) of every kind of input the checker meets, over max(pad, n) variables: genuine answers
    (also undecided ones and incomplete proofs), the mutated proofs of the host test, models with one flipped variable, forged proofs of
    satisfiable instances, and malformed words.  With ``pad`` a sample of them."""
    inst, runs = pm.base_inputs()
    rng = np.random.RandomState(17)
    cases = []

    def add(ic, status, model, region, plen=None):
        cases.append(((max(pad, ic[0]), ic[1]), status, model, np.asarray(region, dtype=np.int32), len(region) if plen is None else plen))

    for A in (0, 12):
        status, models, _, _, _, lemmas, plen = runs[A]
        for i in range(0, len(inst), 1 if A == 0 else 4):
            add(inst[i], status[i], models[i], pm.words(lemmas[i]))
            if A == 0 and status[i] == 1 and i % 2 == 0:
                m = models[i].copy()
                v = int(rng.randint(len(m)))
                m[v] = 1.0 - m[v]
                add(inst[i], 1, m, [])
                for proof in ([], lemmas[i], [[0], [1]]):                            # forged: passed with status 0
                    add(inst[i], 0, models[i], pm.words(proof))
            if A == 0 and status[i] == 0 and i % 4 == 0 and plen[i] > 3:
                add(inst[i], 0, models[i], pm.region(lemmas[i], plen[i] // 2), plen[i])          # an incomplete proof
                add(inst[i], 0, models[i], pm.words(lemmas[i]), -1)
    for c in pm.mutation_cases():
        add(c['inst'], 0, np.zeros(c['inst'][0], dtype=np.float32), pm.words(c['mutated']))
    # malformed words in the last lemma of a genuine proof: a variable id of the next instance (and a negative code), and a length that
    # runs into the next instance's region (and a negative one)
    genuine = [c for c in pm.mutation_cases() if c['kind'] == 'genuine'][:12]
    for c in genuine:
        n = max(pad, c['inst'][0])
        w = pm.words(c['lemmas'])
        at = len(w) - len(c['lemmas'][-1]) - 1                                       # the length word of the last lemma
        for pos, word in ((at + 1, (n + 3) << 1), (at + 1, -2), (at, len(c['lemmas'][-1]) + 2), (at, -1)):
            bad = w.copy()
            bad[pos] = word
            add(c['inst'], 0, np.zeros(c['inst'][0], dtype=np.float32), bad)
    if pad:
        cases = cases[::9] + cases[-4 * len(genuine):]
    add(inst[0], runs[0][0][0], runs[0][1][0], pm.words(runs[0][5][0]))              # a mutated instance is never the last of the batch
    batch = [c[0] for c in cases]
    cols = [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases]
    return (batch,) + cols + (pm.check_all(batch, *cols),)


@pytest.mark.parametrize('pad', [0, CHECK_PAD_N])
def test_checker_equals_the_python_model(pad):
    batch, status, models, regions, plen, want = check_cases(pad)
    assert all(check_on_lds(i) != bool(pad) for i in batch)
    got = run_check(batch, status, models, regions, plen)
    same_check(got, want)
    verdict, fail_at, work = got
    assert set(np.unique(verdict)) == {-1, 0, 1} and (fail_at[verdict != 0] == -1).all() and (fail_at[verdict == 0] >= 0).all()
    assert not work[(np.asarray(status) == -1) | (np.asarray(plen) < 0)].any()


def test_checker_accepts_what_the_search_logged_and_refutes_a_wrong_status():
    "end to end on the device's own buffers: the genuine answers verify; every status swapped 0 <-> 1 is refuted"
    inst, want = pm.base_inputs()
    out = run_proof(inst)
    p = out['prob']
    dev = p.device
    st, model, _, _, proof, off, plen = p.exact_solve_proof()
    verdict, fail_at, work = [t.cpu().numpy() for t in p.exact_check(st, model, proof, off, plen)]
    decided = out['status'] != -1
    assert decided.sum() > 400 and (verdict[decided] == 1).all() and (verdict[~decided] == -1).all() and (fail_at == -1).all()
    swapped = np.where(decided, 1 - out['status'], -1).astype(np.int8)
    verdict = p.exact_check(torch.from_numpy(swapped).to(dev), model, proof, off, plen)[0].cpu().numpy()
    assert (verdict[decided] == 0).all()


# ---- 4. wide lemmas, long proofs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_model(name):
    inst, arena, budget = exact_wide.learn_batches()[name]
    return pm.solve(inst, budget=budget or pm.NO_BUDGET, arena=arena)


@pytest.mark.parametrize('name', ['fan', 'wide-0', 'wide-70'])
def test_wide_lemmas_and_long_proofs(name):
    inst, arena, budget = exact_wide.learn_batches()[name]
    want = wide_model(name)
    longest = max([len(l) for x in want[5] for l in x])
    assert longest > 64 or name == 'fan'
    assert want[3].max() > 64 or name != 'fan'
    out = run_proof(inst, budget=budget, arena=arena)
    same_search(out, want)
    assert (out['plen'] <= out['size']).all() and untouched(out)
    regions = [pm.words(x) for x in want[5]]
    expect = pm.check_all(inst, want[0], want[1], regions, want[6])
    same_check(run_check(inst, want[0], want[1], regions, want[6], prob=out['prob']), expect)
    assert (expect[0][want[0] != -1] == 1).all()


# ---- 5. the checker's budget -------------------------------------------------------------------------------------------------------------
def test_checker_budget():
    inst = [(n, c) for name, n, c in families.exact_cases() if name.startswith('ladder-n60')]
    e = exact_wide.edges(inst)
    assert len(inst) == 5 and (e == e[0]).all()
    run = pm.solve(inst)
    regions = [pm.words(x) for x in run[5]]
    W = np.array([len(r) for r in regions])
    assert (run[0] == 0).any()
    p = problem(inst)
    full = run_check(inst, run[0], run[1], regions, run[6], prob=p)
    same_check(full, pm.check_all(inst, run[0], run[1], regions, run[6]))
    assert (full[0] == 1).all()
    for budget in (1, int(e[0]), 10 * int(e[0])):
        got = run_check(inst, run[0], run[1], regions, run[6], budget=budget, prob=p)
        same_check(got, pm.check_all(inst, run[0], run[1], regions, run[6], budget))
        assert (got[2] < budget + e + W).all()
        done = got[0] != -1
        for g, f in zip(got, full):
            np.testing.assert_array_equal(g[done], f[done])
    assert (run_check(inst, run[0], run[1], regions, run[6], budget=1, prob=p)[0][run[0] == 0] == -1).all()


# ---- 6. determinism and instance-locality ------------------------------------------------------------------------------------------------
def test_deterministic_and_instance_local():
    from pdp import native
    inst, want = pm.base_inputs()
    probe = int(np.argmax(want[0][6]))                                               # the instance with the longest proof
    few = [inst[i] for i in range(0, 420, 9)]
    assert want[0][0][probe] == 0 and len(want[0][5][probe]) > 10

    def answers(arena):
        w = want[arena]
        one = take(w, [probe])
        out = []
        p = problem([inst[probe]])
        for _ in range(2):                                                            # the same problem called twice
            r = run_proof([inst[probe]], arena=arena, prob=p)
            same_search(r, one)
            out.append(run_check([inst[probe]], r['status'], r['models'], r['words'], r['plen'], prob=p))
        for batch, at in (([inst[probe]] + few, 0), (few + [inst[probe]], len(few)), (few[:20] + [inst[probe]] + few[20:], 20)):
            r = run_proof(batch, arena=arena)
            same_search({k: (v[at:at + 1] if k != 'prob' and k != 'proof' and k != 'off' else v) for k, v in r.items()}, one)
            got = run_check(batch, r['status'], r['models'], r['words'], r['plen'], prob=r['prob'])
            out.append(tuple(g[at:at + 1] for g in got))
        return out

    def expected(arena):
        w = want[arena]
        return pm.check_all([inst[probe]], w[0][[probe]], [w[1][probe]], [pm.words(w[5][probe])], w[6][[probe]])

    for arena in (0, 40):
        for g in answers(arena):
            same_check(g, expected(arena))
        assert expected(arena)[0][0] == (1 if want[arena][0][probe] != -1 else -1)
    prev = native.use_build('fast')
    try:
        fast = answers(0)
        same_search(run_proof(inst, arena=40), want[40])
    finally:
        native.use_build(prev)
    for g in fast:
        same_check(g, expected(0))


# ---- 7. hints --------------------------------------------------------------------------------------------------------------------------
def test_hints():
    inst, want = pm.base_inputs()
    base = want[0]
    sat = base[0] == 1
    own = run_proof(inst, hints=[m.copy() for m in base[1]])
    assert not own['plen'][sat].any() and not own['learned'][sat].any() and (own['status'][sat] == 1).all() and untouched(own)
    reads = np.array([exact_model.check_reads(c, m)[0] for (_, c), m in zip(inst, base[1])], dtype=np.int64)
    np.testing.assert_array_equal(own['work'][sat], reads[sat])
    rng = np.random.RandomState(8)
    for frac in (0.3, 0.0):
        hints = []
        for m in base[1]:
            h = rng.randint(0, 2, size=len(m)).astype(np.float32)
            h[rng.rand(len(m)) < frac] = np.nan
            hints.append(h)
        for arena in (0, 40):
            model = pm.solve(inst, hints=hints, arena=arena)
            out = run_proof(inst, hints=hints, arena=arena)
            same_search(out, model)
            regions = [pm.words(x) for x in model[5]]
            got = run_check(inst, out['status'], out['models'], out['words'], out['plen'], prob=out['prob'])
            same_check(got, pm.check_all(inst, model[0], model[1], regions, model[6]))
            assert (got[0][model[0] != -1] == 1).all()


# ---- 8. refusals, and the retry and the alarm of solve_items -------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    items = dataset.random_ksat_items(4, 20, 3, seed=1)
    b = dataset.to_torch(dataset.collate_segment(items), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_solve_proof()
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=p.device)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_check(z(p.B, torch.int8), z(p.V, torch.float32), None, z(p.B + 1, torch.int64), z(p.B, torch.int64))
    p = native.Problem(*args)
    off = torch.arange(p.B + 1, dtype=torch.int64, device=p.device) * 8
    down = off.flip(0).contiguous()
    for kw in (dict(arena=-1), dict(arena=2.5), dict(hints=z(p.V + 1, torch.float32)), dict(proof_off=off.int()), dict(proof_off=off[:-1]),
               dict(proof_off=down), dict(proof_off=off - 1), dict(proof_off=off, proof=z(int(off[-1]), torch.int64)),
               dict(proof_off=off, proof=z(int(off[-1]) - 1, torch.int32))):
        with pytest.raises(ValueError):
            p.exact_solve_proof(**kw)
    st, model, _, _, proof, off, plen = p.exact_solve_proof()
    good = (st, model, proof, off, plen)
    assert (p.exact_check(*good)[0] == 1).all()
    for k, bad in ((0, st.int()), (0, st[:-1]), (1, model.double()), (1, model[:-1]), (2, proof.long()), (2, proof[:int(off[-1]) - 1]), (2, None),
                   (3, off.int()), (3, off.flip(0).contiguous()), (4, plen.int()), (4, plen[:-1])):
        a = list(good)
        a[k] = bad
        with pytest.raises(ValueError):
            p.exact_check(*a)
    # solve_items(certify=True): regions that are too small cost one more run, never an answer
    inst = [pm.base_inputs()[0][i] for i in range(0, 420, 7)] + [lm.thrash(6)]
    raw = [exact.raw_item(n, c, name='inst%d' % i) for i, (n, c) in enumerate(inst)]
    plain = exact.solve_items(raw, learn=True)
    assert set(np.unique(plain[0])) == {0, 1}
    monkeypatch.setattr(native, 'PROOF_WORDS_PER_LITERAL', 0)
    status, models, work, verdict, lemmas = exact.solve_items(raw, certify=True, proofs=True)
    monkeypatch.undo()
    np.testing.assert_array_equal(status, plain[0])
    np.testing.assert_array_equal(work, plain[2])
    assert (verdict == 1).all()
    want = pm.solve(inst)
    assert sum(len(x) > 0 for x in want[5]) > 10
    assert all((l == w if s == 0 else l is None) for l, w, s in zip(lemmas, want[5], status))
    assert exact.solve_items(raw, certify=True)[3].tolist() == verdict.tolist()
    assert exact.label_clause_lists(inst[:5], certify=True) == [bool(s) for s in status[:5]]
    with pytest.raises(ValueError):
        exact.solve_items(raw, proofs=True)
    # a checker that refutes an unsatisfiable instance's genuine proof: no label, an error that names the instance
    victim = int(np.nonzero(status == 0)[0][3])
    real = native.Problem.exact_check

    def lying(self, *a, **kw):
        verdict, fail_at, wk = real(self, *a, **kw)
        verdict[victim], fail_at[victim] = 0, 2
        return verdict, fail_at, wk

    monkeypatch.setattr(native.Problem, 'exact_check', lying)
    with pytest.raises(RuntimeError, match=r'instance %d \(inst%d\).*lemma 2' % (victim, victim)):
        exact.solve_items(raw, certify=True)


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_complete_certify(tmp_path):
    from test_sharded_gpu import _run
    ddir = os.path.join(REPO, 'tests', 'golden', 'dimacs20')
    argv = [PDP_YAML, ddir, '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    learn, _ = _run(argv + ['--complete-learn'], 1, str(tmp_path / 'learn.jsonl'), 0)
    cert, _ = _run(argv + ['--complete-certify'], 1, str(tmp_path / 'cert.jsonl'), 0)
    a, b = [json.loads(l) for l in learn], [json.loads(l) for l in cert]
    assert len(a) == 20
    for r, s in zip(a, b):
        assert list(s) == list(r) + ['certified'] and list(s).index('certified') == list(s).index('work') + 1
        assert {k: v for k, v in s.items() if k != 'certified'} == r
        assert s['certified'] == (1 if s['complete'] != -1 else -1)
    assert {r['complete'] for r in b} <= {0, 1}


def test_cli_dimacs2json_certified(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    from pdp import exact
    ddir = str(tmp_path / 'cnf')                                                     # tests/golden/dimacs20 has no unsatisfiable instance
    os.makedirs(ddir)
    inst, runs = pm.base_inputs()
    pick = [i for i in range(420) if [] not in inst[i][1]]
    pick = [i for i in pick if runs[0][0][i] == 0][:4] + [i for i in pick if runs[0][0][i] == 1][:3]
    for k, (n, clauses) in enumerate([inst[i] for i in pick] + [lm.thrash(3), lm.thrash(7)]):
        with open(os.path.join(ddir, 'f%02d.cnf' % k), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    out, plain, pdir = str(tmp_path / 'c.json'), str(tmp_path / 'l.json'), str(tmp_path / 'proofs')
    args = vars(dimacs2json.cli_parser().parse_args([ddir, out, '--label', 'exact-certified', '--proof-dir', pdir]))
    dimacs2json.convert_directory(args['in_dir'], args['out_file'], args['simplify'], args['positive'], args['label'], args['budget'], args['proof_dir'])
    dimacs2json.convert_directory(ddir, plain, label='exact-learn')
    assert open(out).read() == open(plain).read()                                    # every decided answer is certified: the same labels
    names = sorted(f for f in os.listdir(ddir) if os.path.splitext(f)[1].lower() in ('.dimacs', '.cnf'))
    labels = {}
    for name in names:
        n, m, sv, ci = dimacs2json.compact_instance(os.path.join(ddir, name))
        clauses = [[] for _ in range(m)]
        for l, c in zip(sv, ci):
            clauses[int(c) - 1].append(int(l))
        labels[name] = exact.is_sat(n, clauses, learn=True)
        drat = os.path.join(pdir, name + '.drat')
        assert os.path.exists(drat) == (labels[name] is False)
        if labels[name] is False:
            lines = open(drat).read().splitlines()
            assert lines[-1] == '0'
            lemmas = [[((abs(int(t)) - 1) << 1) | (int(t) < 0) for t in l.split()[:-1]] for l in lines[:-1]]
            w = pm.words(lemmas)
            assert pm.check(n, clauses, 0, None, w, len(w))[:2] == (1, -1)
    assert sorted(os.listdir(pdir)) == sorted(name + '.drat' for name in names if labels[name] is False)
    assert sum(v is False for v in labels.values()) >= 6 and sum(v is True for v in labels.values()) >= 3
