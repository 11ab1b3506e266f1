"""The backward check of a proof on the GPU (pdp_exact_trim; Problem.exact_trim, exact.trimmed / core_clauses,
exact.solve_items(certify=True, cores=True), satyr.py --complete-core, dimacs2json.py --core): equal to its Python statement
(tests/exact_trim_model.py) in all seven outputs, byte for byte over the whole keep buffer, on both routes, past one wave's width, with one
wave running instance after instance, on a relaunched handle and in both builds; the cores and the trimmed proofs judged by the GPU's own
search and forward checker (T3, T4); refusals; the command lines."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import exact_model
import exact_proof_model as pm
import exact_reuse as xr
import exact_trim_model as tm
import exact_wide as xw
import exact_learn_model as lm
from helpers import REPO
from test_exact_learn_gpu import PDP_YAML, problem
from test_exact_wide_gpu import LEARN_BATCHES

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
KEEP_SENTINEL = 0x5A
PAD_N = xw.PLAIN_PAD_N       # 21 bytes of slab per variable, as the plain search: 2400 variables are past 48 KiB


def on_lds(inst):
    "ext_lds_layout of csrc/pdp_exact.hip: 8 n + 4 n + 4 n + 4 (n + 1) + 2 e + 2 (m + 1) + n bytes, up to 48 KiB"
    n, c = inst
    e = sum(len(x) for x in c)
    n = max([n] + [abs(l) for x in c for l in x])
    return ((21 * n + 4 + 2 * e + 2 * (len(c) + 1) + 15) & ~15) <= 48 * 1024 and e <= 65535 and n < 32768


def run_trim(inst, status, regions, plen, budget=0, prob=None):
    """one call of exact_trim on sentinel-filled buffers: dict of the seven outputs as numpy arrays, the device tensors and the problem;
    ``regions``: the int32 words of every instance's region"""
    p = problem(inst) if prob is None else prob
    dev = p.device
    off = np.concatenate([[0], np.cumsum([len(r) for r in regions])]).astype(np.int64)
    proof = np.concatenate([np.asarray(r, dtype=np.int32) for r in regions] + [np.full(5, SENTINEL, dtype=np.int32)])
    t = dict(status=torch.from_numpy(np.asarray(status, dtype=np.int8)).to(dev), proof=torch.from_numpy(proof).to(dev),
             off=torch.from_numpy(off).to(dev), plen=torch.from_numpy(np.asarray(plen, dtype=np.int64)).to(dev))
    t['keep'] = torch.full((len(proof),), KEEP_SENTINEL, dtype=torch.int8, device=dev)
    out = p.exact_trim(t['status'], t['proof'], t['off'], t['plen'], budget, keep=t['keep'])
    assert out[4] is t['keep']
    names = ('verdict', 'fail_at', 'work', 'core', 'keep', 'n_core', 'n_keep')
    got = {k: v.cpu().numpy() for k, v in zip(names, out)}
    got.update(prob=p, dev=t, dev_out=dict(zip(names, out)), off=off)
    return got


def same_trim(got, want, regions):
    "all seven outputs equal to tm.trim_all's: core over the whole problem, keep over the whole buffer (the sentinel where nothing is written)"
    verdict, fail_at, work, cores, keeps, n_core, n_keep = want
    np.testing.assert_array_equal(got['verdict'], verdict)
    np.testing.assert_array_equal(got['fail_at'], fail_at)
    np.testing.assert_array_equal(got['work'], work)
    np.testing.assert_array_equal(got['n_core'], n_core)
    np.testing.assert_array_equal(got['n_keep'], n_keep)
    np.testing.assert_array_equal(got['core'], np.concatenate(cores))
    expect = np.full(len(got['keep']), KEEP_SENTINEL, dtype=np.int8)
    for a, k in zip(got['off'][:-1], keeps):
        if k is not None:
            expect[a:a + len(k)] = k
    np.testing.assert_array_equal(got['keep'], expect)


def gpu_t3_t4(inst, got):
    """T3 and T4 by the GPU's own kernels: the core sub-instances of the verdict-1 instances are all unsatisfiable for pdp_exact_solve, and
    pdp_exact_check accepts exact.trimmed's words against them"""
    from pdp import exact
    t, o = got['dev'], got['dev_out']
    words, toff = exact.trimmed(t['proof'], t['off'], t['plen'], o['keep'])
    toff = toff.cpu().numpy()
    ok = np.nonzero(got['verdict'] == 1)[0]
    assert len(ok) > 20
    counts = [len(c) for _, c in inst]
    cores = exact.core_clauses(o['core'], counts)
    sub = [(inst[b][0], [inst[b][1][k] for k in cores[b]]) for b in ok]
    assert all(len(c) == got['n_core'][b] for (_, c), b in zip(sub, ok))
    p = problem(sub)
    st, model, _ = p.exact_solve()
    assert (st.cpu().numpy() == 0).all()
    words = words.cpu().numpy()
    regions = [words[toff[b]:toff[b + 1]] for b in ok]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in regions])]).astype(np.int64)).to(p.device)
    proof = torch.from_numpy(np.concatenate(regions + [np.zeros(1, dtype=np.int32)])).to(p.device)
    verdict, fail_at, _ = p.exact_check(st, model, proof, off, off[1:] - off[:-1])
    assert (verdict.cpu().numpy() == 1).all() and (fail_at.cpu().numpy() == -1).all()
    # the kept lemmas are the marked ones, in order
    for b, r in zip(ok, regions):
        assert len(pm.parse(r)) == got['n_keep'][b]


# ---- 1. the base inputs and the mutations ------------------------------------------------------------------------------------------------
def test_base_inputs_equal_the_python_model():
    inst, regions, plen, want, _ = tm.base_cases()
    assert all(on_lds(i) for i in inst)
    got = run_trim(inst, np.zeros(len(inst), dtype=np.int8), regions, plen)
    same_trim(got, want, regions)
    assert (got['verdict'] == 1).all()
    gpu_t3_t4(inst, got)


def test_mutations_equal_the_python_model():
    inst, status, regions, plen, want, _, forward = tm.mutation_batch()
    got = run_trim(inst, status, regions, plen)
    same_trim(got, want, regions)
    assert set(np.unique(got['verdict'])) == {-1, 0, 1}
    assert (got['fail_at'][got['verdict'] != 0] == -1).all() and (got['fail_at'][got['verdict'] == 0] >= 0).all()
    gpu_t3_t4(inst, got)
    # T1 and T2 against the GPU's forward checker on the same buffers
    p, t = got['prob'], got['dev']
    fwd = p.exact_check(t['status'], torch.zeros(p.V, dtype=torch.float32, device=p.device), t['proof'], t['off'], t['plen'])[0].cpu().numpy()
    judged = (status == 0) & (got['verdict'] != -1)
    assert (got['verdict'][judged & (fwd == 1)] == 1).all() and (fwd[judged & (got['verdict'] == 0)] == 0).all()
    assert (judged & (fwd == 0) & (got['verdict'] == 1)).any()


def test_mutations_in_the_fast_build():
    from pdp import native
    inst, status, regions, plen, want, _, _ = tm.mutation_batch()
    prev = native.use_build('fast')
    try:
        same_trim(run_trim(inst, status, regions, plen), want, regions)
    finally:
        native.use_build(prev)


# ---- 2. past one wave's width, on both routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [0, PAD_N])
def test_wide_refutations(pad):
    inst, regions, plen, want, stats = tm.wide_cases()
    batch = [(max(pad, n), c) for n, c in inst]
    assert all(on_lds(i) != bool(pad) for i in batch)
    got = run_trim(batch, np.zeros(len(batch), dtype=np.int8), regions, plen)
    same_trim(got, want, regions)
    assert (got['verdict'] == 1).all() and got['n_keep'].max() > 128


@pytest.mark.parametrize('pad', [0, PAD_N])
@pytest.mark.parametrize('name', LEARN_BATCHES)
def test_learn_batches(name, pad):
    "the wide instances of the learning search with their own proofs: as answered, and every proof passed as one of unsatisfiability"
    from test_exact_proof_gpu import wide_model
    inst, _, _ = xw.learn_batches()[name]
    run = wide_model(name)
    batch = [(max(pad, n), c) for n, c in inst]
    assert all(on_lds(i) != bool(pad) for i in batch)
    regions = [pm.words(x) for x in run[5]]
    p = None
    for status in (run[0], np.zeros(len(inst), dtype=np.int8)):
        want = tm.trim_all(batch, status, regions, run[6])
        got = run_trim(batch, status, regions, run[6], prob=p)
        same_trim(got, want, regions)
        p = got['prob']
    assert (got['verdict'] == 0).sum() >= 4 and (got['verdict'] == 1).sum() >= 4    # a satisfiable instance's lemmas refute nothing
    assert max(len(l) for x in run[5] for l in x) > 64 or name == 'fan'


def test_both_routes_in_one_batch():
    mixed, _ = xr.routes()
    run = xr.routes_proof(0)
    assert 0 < sum(on_lds(i) for i in mixed) < len(mixed)
    regions = [pm.words(x) for x in run[5]]
    status = np.where(run[0] == 1, 0, run[0]).astype(np.int8)                      # the satisfiable ones too: their lemmas refute nothing
    want = tm.trim_all(mixed, status, regions, run[6])
    got = run_trim(mixed, status, regions, run[6])
    same_trim(got, want, regions)
    assert set(np.unique(got['verdict'])) >= {0, 1}
    big = np.array([not on_lds(i) for i in mixed])
    assert (got['verdict'][big] == 1).any() and (got['verdict'][~big] == 1).any()


# ---- 3. one wave, instance after instance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [1, 2])
def test_crossing_at_a_lowered_grid(monkeypatch, grid):
    """crossing(): every 4-byte array of a successor is longer than its predecessor's, so it lies over the predecessor's literals, offsets and
    values; the request words, reasons, batches and value bytes of an instance must not depend on what they find"""
    inst = xr.crossing()
    run = xr.cross_proof(0)
    assert all(on_lds(i) for i in inst) and (run[0] == 0).sum() >= 5
    regions = [pm.words(x) for x in run[5]]
    status = np.where((run[0] == 1) & (np.arange(len(inst)) % 2 == 0), 0, run[0]).astype(np.int8)    # of the satisfiable ones, every other is judged
    want = tm.trim_all(inst, status, regions, run[6])
    monkeypatch.setenv('PDP_EXACT_GRID', str(grid))
    got = run_trim(inst, status, regions, run[6])
    assert got['prob'].exact_last_grid() == grid
    same_trim(got, want, regions)
    again = run_trim(inst, status, regions, run[6], prob=got['prob'])               # the same handle once more: the HBM-side state too
    assert again['prob'].exact_last_grid() == grid
    same_trim(again, want, regions)
    monkeypatch.delenv('PDP_EXACT_GRID')
    full = run_trim(inst, status, regions, run[6], prob=got['prob'])
    assert full['prob'].exact_last_grid() == len(inst)
    same_trim(full, want, regions)
    assert set(np.unique(got['verdict'])) == {-1, 0, 1}


def test_a_larger_proof_buffer_on_the_same_handle():
    "two calls on one handle, the second with a larger proof buffer and other regions: nothing is kept from the first"
    inst, regions, plen, want, _ = tm.base_cases()
    pick = list(range(0, len(inst), 7))
    batch = [inst[i] for i in pick]
    take = lambda w: (w[0][pick], w[1][pick], w[2][pick], [w[3][i] for i in pick], [w[4][i] for i in pick], w[5][pick], w[6][pick])
    small = [regions[i] for i in pick]
    first = run_trim(batch, np.zeros(len(batch), dtype=np.int8), small, plen[pick])
    same_trim(first, take(want), small)
    large = [np.concatenate([r, np.full(3 * len(r) + 11, 9, dtype=np.int32)]) for r in small]     # the proofs stand elsewhere, with words after them
    second = run_trim(batch, np.zeros(len(batch), dtype=np.int8), large, plen[pick], prob=first['prob'])
    assert len(second['keep']) > 3 * len(first['keep'])
    same_trim(second, take(want), large)


def test_budget():
    inst, regions, plen, want, _ = tm.base_cases()
    pick = np.argsort(want[2])[-60:]
    batch = [inst[i] for i in pick]
    reg = [regions[i] for i in pick]
    e, W = xw.edges(batch), np.array([len(r) for r in reg])
    p = None
    for budget in (1, int(np.median(want[2][pick])) // 2, int(want[2][pick].max())):
        got = run_trim(batch, np.zeros(len(batch), dtype=np.int8), reg, plen[pick], budget=budget, prob=p)
        p = got['prob']
        same_trim(got, tm.trim_all(batch, np.zeros(len(batch), dtype=np.int8), reg, plen[pick], budget), reg)
        assert (got['work'] < budget + 3 * (e + W)).all()
        assert budget > 1 or (got['verdict'] == -1).all()
    assert (got['verdict'] == 1).all()


# ---- 4. refusals and solve_items -----------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from pdp import native
    from pdp.factorgraph import dataset
    items = dataset.random_ksat_items(4, 20, 3, seed=1)
    b = dataset.to_torch(dataset.collate_segment(items), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=p.device)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_trim(z(p.B, torch.int8), None, z(p.B + 1, torch.int64), z(p.B, torch.int64))
    p = native.Problem(*args)
    st, model, _, _, proof, off, plen = p.exact_solve_proof()
    good = (st, proof, off, plen)
    out = p.exact_trim(*good)
    assert (out[0].cpu().numpy() == np.where(st.cpu().numpy() == 0, 1, -1)).all() and out[4].numel() == proof.numel() and out[3].numel() == p.F
    for k, bad in ((0, st.int()), (0, st[:-1]), (1, proof.long()), (1, proof[:int(off[-1]) - 1]), (1, None), (2, off.int()), (2, off[:-1]),
                   (2, off.flip(0).contiguous()), (2, off - 1), (3, plen.int()), (3, plen[:-1])):
        a = list(good)
        a[k] = bad
        with pytest.raises(ValueError):
            p.exact_trim(*a)
    for keep in (torch.zeros(proof.numel() + 1, dtype=torch.int8, device=p.device), torch.zeros(proof.numel(), dtype=torch.int32, device=p.device),
                 torch.zeros(proof.numel(), dtype=torch.int8)):
        with pytest.raises(ValueError):
            p.exact_trim(*good, keep=keep)
    # no proof words at all: nothing to keep
    none = p.exact_trim(st, None, torch.zeros(p.B + 1, dtype=torch.int64, device=p.device), torch.zeros(p.B, dtype=torch.int64, device=p.device))
    assert none[4] is None and (none[0].cpu().numpy()[st.cpu().numpy() != 0] == -1).all()


def test_solve_items_with_cores(monkeypatch):
    from pdp import exact, native
    inst = [pm.base_inputs()[0][i] for i in range(0, 420, 7)] + [lm.thrash(6), (3, [[1], [], [2]]), (2, [[], []])]
    raw = [exact.raw_item(n, c, name='inst%d' % i) for i, (n, c) in enumerate(inst)]
    plain = exact.solve_items(raw, certify=True, proofs=True)
    want = pm.solve(inst)

    def judge(out):
        status, models, work, verdict, lemmas, cores = out
        np.testing.assert_array_equal(status, plain[0])
        np.testing.assert_array_equal(work, plain[2])
        assert (verdict == 1).all() and (status == 0).sum() > 10
        for i, (n, c) in enumerate(inst):
            if status[i] != 0:
                assert lemmas[i] is None and cores[i] is None
                continue
            w = pm.words(want[5][i])
            v, f, _, core, keep = tm.trim(n, c, w, len(w))
            assert v == 1 and list(cores[i]) == list(np.nonzero(core)[0]) and lemmas[i] == tm.kept(w, len(w), keep)

    judge(exact.solve_items(raw, certify=True, cores=True))
    monkeypatch.setattr(native, 'PROOF_WORDS_PER_LITERAL', 0)                       # no proof fits: every one is logged again
    judge(exact.solve_items(raw, certify=True, cores=True))
    monkeypatch.undo()
    with pytest.raises(ValueError):
        exact.solve_items(raw, cores=True)
    with pytest.raises(ValueError):
        exact.solve_items(raw, learn=True, cores=True)
    # an instance without a literal is answered on the host: its first empty clause is its core
    only = exact.solve_items([exact.raw_item(2, [[], []])], certify=True, cores=True)
    assert only[0].tolist() == [0] and only[4] == [[]] and list(only[5][0]) == [0]
    # a backward check that refutes a genuine proof: no label, an error that names the instance
    victim = int(np.nonzero(plain[0] == 0)[0][3])
    real = native.Problem.exact_trim

    def lying(self, *a, **kw):
        out = list(real(self, *a, **kw))
        out[0][victim], out[1][victim] = 0, 2
        return tuple(out)

    monkeypatch.setattr(native.Problem, 'exact_trim', lying)
    with pytest.raises(RuntimeError, match=r'instance %d \(inst%d\).*lemma 2' % (victim, victim)):
        exact.solve_items(raw, certify=True, cores=True)


# ---- 5. the command lines --------------------------------------------------------------------------------------------------------------------
def cnf_dir(tmp_path):
    "a directory of DIMACS files: unsatisfiable and satisfiable small instances and two of the thrash family"
    ddir = str(tmp_path / 'cnf')                                                     # tests/golden/dimacs20 has no unsatisfiable instance
    os.makedirs(ddir)
    inst, runs = pm.base_inputs()
    pick = [i for i in range(420) if [] not in inst[i][1]]
    pick = [i for i in pick if runs[0][0][i] == 0][:4] + [i for i in pick if runs[0][0][i] == 1][:3]
    for k, (n, clauses) in enumerate([inst[i] for i in pick] + [lm.thrash(3), lm.thrash(7)]):
        with open(os.path.join(ddir, 'f%02d.cnf' % k), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    return ddir


def loader_clauses(path):
    "(variables, clauses) of a file as the loader holds them"
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    n, m, sv, ci = dimacs2json.compact_instance(path)
    clauses = [[] for _ in range(m)]
    for l, c in zip(sv, ci):
        clauses[int(c) - 1].append(int(l))
    return n, clauses


def test_cli_complete_core(tmp_path):
    from test_sharded_gpu import _run
    ddir = cnf_dir(tmp_path)
    argv = [PDP_YAML, ddir, '100', '-d', '--rng', 'philox', '-s', '7', '--complete', '--complete-certify']
    cert, _ = _run(argv, 1, str(tmp_path / 'cert.jsonl'), 0)
    core, _ = _run(argv + ['--complete-core'], 1, str(tmp_path / 'core.jsonl'), 0)
    a, b = [json.loads(l) for l in cert], [json.loads(l) for l in core]
    assert len(a) == 9 and sum(r['complete'] == 0 for r in a) >= 6
    for r, s in zip(a, b):
        assert 'core' not in r
        if r['complete'] == 0:
            assert list(s) == list(r) + ['core'] and list(s).index('core') == list(s).index('certified') + 1
            n, clauses = loader_clauses(os.path.join(ddir, r['ID']))
            assert s['core'] == sorted(set(s['core'])) and 0 < len(s['core']) <= len(clauses)
            assert exact_model.search(n, [clauses[k] for k in s['core']])[0] == 0
        else:
            assert list(s) == list(r)
        assert {k: v for k, v in s.items() if k != 'core'} == r and s['certified'] == 1
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import satyr
    with pytest.raises(SystemExit):
        satyr.main([PDP_YAML, ddir, '100', '-d', '--complete', '--complete-core'])


def test_cli_dimacs2json_core(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    ddir = cnf_dir(tmp_path)
    outs = {}
    for key, extra in (('plain', []), ('core', ['--core'])):
        out, pdir = str(tmp_path / (key + '.json')), str(tmp_path / (key + '-proofs'))
        args = vars(dimacs2json.cli_parser().parse_args([ddir, out, '--label', 'exact-certified', '--proof-dir', pdir] + extra))
        dimacs2json.convert_directory(args['in_dir'], args['out_file'], args['simplify'], args['positive'], args['label'], args['budget'],
                                      args['proof_dir'], args['core'])
        outs[key] = (open(out).read(), pdir)
    assert outs['plain'][0] == outs['core'][0]                                       # the same labels
    names = sorted(f for f in os.listdir(ddir))
    unsat = 0
    for name in names:
        n, clauses = loader_clauses(os.path.join(ddir, name))
        run = pm.search(n, clauses)
        drat, core = os.path.join(outs['core'][1], name + '.drat'), os.path.join(outs['core'][1], name + '.core.cnf')
        full = os.path.join(outs['plain'][1], name + '.drat')
        assert os.path.exists(drat) == os.path.exists(core) == os.path.exists(full) == (run[0] == 0)
        if run[0] != 0:
            continue
        unsat += 1
        from pdp import exact
        assert open(full).read() == '\n'.join(exact.drat_lines(run[5])) + '\n'     # without the flag: the whole log, as before
        # the pair is self-contained: the .core.cnf is read back as it stands, the .drat is a proof of it
        cn, cc = dimacs2json.parse_dimacs(core)
        assert cn == n and all(c in clauses for c in cc)
        lines = open(drat).read().splitlines()
        assert lines[-1] == '0'
        lemmas = [[((abs(int(t)) - 1) << 1) | (int(t) < 0) for t in l.split()[:-1]] for l in lines[:-1]]
        w = pm.words(lemmas)
        assert pm.check(cn, cc, 0, None, w, len(w))[:2] == (1, -1)
        assert tm.trim(cn, cc, w, len(w))[0] == 1 and exact_model.search(cn, cc)[0] == 0
        assert len(lemmas) <= len(run[5]) and len(cc) <= len(clauses)
    assert unsat >= 6
    assert sorted(os.listdir(outs['plain'][1])) == sorted(f for f in os.listdir(outs['core'][1]) if not f.endswith('.core.cnf'))
    with pytest.raises(ValueError):
        dimacs2json.convert_directory(ddir, str(tmp_path / 'x.json'), label='exact-learn', core=True)
