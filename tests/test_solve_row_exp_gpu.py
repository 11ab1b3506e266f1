"""The LDS-resident solver takes exp of the two row sums of a variable once per variable (R1) and E2 reads them from scratch arrays that the
cold routines -- decimation, simplification, the Reinforce step -- use as well.  The hazard is a stale or clobbered per-variable value, so
every case here aims at a sweep that directly follows a user of those arrays, or at an end of the exp's range, and compares the call with
the oracle's loop by array_equal: q, fs, edge mask, solution, active masks and the executed sweeps, NaN positions included.  What a case
needs of the oracle's trajectory (a decimation of each kind, a row sum below the exp's clamp, a NaN) is asserted, never skipped."""
import numpy as np
import pytest
import torch

import families
from helpers import random_batch, load_golden
from test_hip_ops import t, npy, make_pair

pytestmark = pytest.mark.gpu


def oracle_forward(oracle, b, T, tol, t_max):
    op = oracle.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], 1)
    return op, op.forward('p-d-p', T, local_search_iterations=0, tolerance=tol, t_max=t_max, seed=5, trace=True, trace_float=True)


def solve_and_compare(oracle, b, T, tol, t_max, ref=None, isolated=False, expect_lds=True):
    from pdp import native
    op, res = ref if ref is not None else oracle_forward(oracle, b, T, tol, t_max)
    hp = native.Problem(t(b['graph_map']), t(b['batch_variable_map']), t(b['batch_function_map']), t(b['edge_feature']))
    hp.simplify()
    q = torch.full((hp.E, 3), 1.0, device='cuda:0') / 3.0
    fs = torch.zeros(hp.E, 2, device='cuda:0'); fs[:, 0] = 0.5
    am = torch.ones(hp.B, dtype=torch.uint8, device='cuda:0')
    iters, used_lds = hp.sp_solve(q, fs, am, native.Decimator(hp), T, tol, t_max, isolate_instances=isolated)
    assert used_lds == expect_lds
    it = res['iterations_run']
    assert iters == it
    np.testing.assert_array_equal(npy(am), res['trace_active_mask'][it - 1])
    np.testing.assert_array_equal(npy(hp.active_variables)[:, 0], res['trace_active_var'][it - 1])
    np.testing.assert_array_equal(npy(hp.active_functions)[:, 0], res['trace_active_fn'][it - 1])
    np.testing.assert_array_equal(npy(hp.solution), res['trace_solution'][it - 1])
    np.testing.assert_array_equal(npy(q), res['q'])
    np.testing.assert_array_equal(npy(fs), res['fs'])
    hp.refresh_edge_mask()
    np.testing.assert_array_equal(npy(hp.edge_mask)[:, 0], op.refresh_edge_mask()[0])
    return hp, res


# ---- what happened in the oracle's run, from its trajectory ------------------------------------------------------------------------------
def decimation_events(b, res):
    """[(sweep, instance, kind)] of the oracle's decimations.  A decimation fixes the arg-max variable and switches the clauses it satisfies
    off; 'fast' if that leaves no unit clause and no pure variable (the neighbourhood path of lds_decimate ends there), 'unit' if an active
    clause is left with one active variable (the hand-over to d_simplify), 'pure' if only a pure variable appears (d_peel).  With several
    variables fixed in one sweep the arg-max one is not recorded: the event counts only if every candidate gives the same kind."""
    ev, ec = b['graph_map'][0].astype(np.int64), b['graph_map'][1].astype(np.int64)
    sg = b['edge_feature'].reshape(-1)
    inst_of_var = b['batch_variable_map'].astype(np.int64)
    it = res['iterations_run']
    av, af, sol = res['trace_active_var'], res['trace_active_fn'], res['trace_solution']
    out = []
    for s in range(1, it):
        fixed = np.nonzero((av[s - 1] == 1) & (av[s] == 0))[0]
        for i in np.unique(inst_of_var[fixed]):
            if not res['trace_active_mask'][s - 1][i]:
                continue
            mine = fixed[inst_of_var[fixed] == i]
            kinds = set()
            for li in mine:
                a_v, a_f = av[s - 1].copy(), af[s - 1].copy()
                a_v[li] = 0
                lit_true = (ev == li) & ((sg > 0) == (sol[s][li] > 0.5))
                a_f[ec[lit_true]] = 0
                live = (a_v[ev] == 1) & (a_f[ec] == 1)
                width = np.bincount(ec[live], minlength=a_f.size)
                unit = bool(((width == 1) & (a_f == 1)).any())
                pos = np.bincount(ev[live & (sg > 0)], minlength=a_v.size); neg = np.bincount(ev[live & (sg < 0)], minlength=a_v.size)
                pure = bool((((pos == 0) | (neg == 0)) & (a_v == 1) & (inst_of_var == i)).any())
                kinds.add('unit' if unit else ('pure' if pure else 'fast'))
            if len(kinds) == 1:
                out.append((s, int(i), kinds.pop()))
    return out


def row_sums(b, res, s):
    "P / N of every variable as sweep s of the oracle's run forms them: sums of log(max(1 - eta, 1e-40)) * edge mask over the edges of each sign"
    ev, ec = b['graph_map'][0].astype(np.int64), b['graph_map'][1].astype(np.int64)
    sg = b['edge_feature'].reshape(-1)
    eta = np.full(ev.size, 0.5, np.float32) if s == 0 else res['trace_fs'][s - 1][:, 0]
    y = np.log(np.maximum(1.0 - eta.astype(np.float64), 1e-40))
    if s > 0:
        y = y * ((res['trace_active_var'][s - 1][ev] == 1) & (res['trace_active_fn'][s - 1][ec] == 1))
    V = b['batch_variable_map'].size
    return np.bincount(ev[sg > 0], weights=y[sg > 0], minlength=V), np.bincount(ev[sg < 0], weights=y[sg < 0], minlength=V)


# ---- sweeps behind the users of the scratch arrays ---------------------------------------------------------------------------------------
DECIMATING = dict(batch=96, n=40, k=3, m=140, seed=900)


@pytest.mark.parametrize('chunk', [None, '7'])
def test_sweeps_behind_every_kind_of_decimation(oracle, monkeypatch, chunk):
    """alpha = 3.5, n = 40: instances converge and are decimated sweep after sweep, so R1 / E2 run right behind the scorer, the neighbourhood
    path, d_simplify (unit clause) and d_peel (pure variable), and behind the mask refresh that follows each of them"""
    if chunk:
        monkeypatch.setenv('PDP_SOLVE_CHUNK', chunk)
    b = random_batch(**DECIMATING)
    ref = oracle_forward(oracle, b, 80, 0.05, 8)
    events = decimation_events(b, ref[1])
    kinds = {k for _, _, k in events}
    assert {'fast', 'unit', 'pure'} <= kinds, kinds
    # decimations in consecutive sweeps of ONE instance: the sweep behind a decimation is itself followed by one
    by_inst = {}
    for s, i, _ in events:
        by_inst.setdefault(i, set()).add(s)
    longest = max(max(sum(1 for d in range(20) if all(s + j in ss for j in range(d + 1))) for s in ss) for ss in by_inst.values())
    assert longest >= 4, longest
    assert ref[1]['iterations_run'] >= 60 and not np.isnan(ref[1]['fs']).any()
    solve_and_compare(oracle, b, 80, 0.05, 8, ref=ref)


@pytest.mark.parametrize('tol', [0.02, 0.05])
def test_exact_pass_close_to_the_tolerance(oracle, tol):
    """P5b (the exact smooth maximum of the variables whose bounds straddle the tolerance) uses xv1 and the |delta eta| array between E2 and the
    next R1: a batch whose instances cross the tolerance at different sweeps, with and without decimations behind the crossing"""
    b = random_batch(batch=120, n=50, k=3, m=190, seed=4100)
    ref = oracle_forward(oracle, b, 70, tol, 12)
    assert (ref[1]['trace_active_var'][ref[1]['iterations_run'] - 1] == 0).sum() > 0          # tolerance crossings did lead to decimations
    solve_and_compare(oracle, b, 70, tol, 12, ref=ref)


# ---- the replay instantiation and the adopted poison -------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk,adopt', [(None, True), ('7', True), (None, False), ('7', False)])
def test_poisoned_headline_batch(oracle, monkeypatch, chunk, adopt):
    """the golden poisoned batch of the headline family (four instances whose surveys turn NaN): pass 1 adopts the poison or the replay
    instantiation redoes the instances with an event behind it -- both read per-variable exps that their own R1 wrote"""
    from pdp.factorgraph import dataset
    if chunk:
        monkeypatch.setenv('PDP_SOLVE_CHUNK', chunk)
    if not adopt:
        monkeypatch.setenv('PDP_SOLVE_NO_ADOPT', '1')
    d = load_golden('headline_n200_poison')
    n, mcl, T = [int(x) for x in d['meta'][:3]]
    items = []
    for sd in d['seeds']:
        items += dataset.random_ksat_items(1, n, 3, m=mcl, seed=int(sd))
    b = dataset.collate_segment(items)
    ref = oracle_forward(oracle, b, T, 0.02, 100)
    assert np.isnan(ref[1]['fs']).any() and families.first_nan_sweep(ref[1]) > 0
    hp, _ = solve_and_compare(oracle, b, T, 0.02, 100, ref=ref)
    if not adopt:
        assert hp.last_solve_stats['replays'] >= 1


# ---- the ends of the exp's range ---------------------------------------------------------------------------------------------------------
def _lopsided_hub(rng, pos, neg, n=60):
    "variable 1 in `pos` clauses as a positive and `neg` clauses as a negative literal, the other literals uniform"
    clauses = []
    for j in range(pos + neg):
        a, c = rng.choice(np.arange(2, n + 1), size=2, replace=False)
        clauses.append([1 if j < pos else -1, int(a) * (1 if rng.rand() < 0.5 else -1), int(c) * (1 if rng.rand() < 0.5 else -1)])
    return n, clauses


def _range_batch():
    rng = np.random.RandomState(515)
    inst = [families.ladder(np.random.RandomState(516), 40, 3.5),
            _lopsided_hub(rng, 400, 24),                       # P = 400 log 0.5 = -277 in the first sweep, N = -17: exp(P) is the unclamped branch's +0
            families.ladder(np.random.RandomState(517), 40, 3.5),              # (gets five variables without an edge below)
            _lopsided_hub(rng, 24, 400),
            _lopsided_hub(rng, 400, 400),                      # both sums below the clamp: 0 / 0 in the normalisation, a NaN survey two sweeps later
            families.ladder(np.random.RandomState(518), 50, 3.5)]
    from pdp.factorgraph import dataset
    items = [dataset.instance_from_clauses(n, c, label=-1, name='range%d' % i) for i, (n, c) in enumerate(families.anchored(inst))]
    # the loader compacts unused variables away (as the reference does); five variables without an edge behind the used ones of instance 2:
    # both row sums +0, both exps 1
    items[2] = (items[2][0] + 5,) + tuple(items[2][1:])
    return dataset.collate_segment(items)


@pytest.mark.parametrize('T', [1, 2, 8])
def test_row_sums_at_the_ends_of_the_exp_range(oracle, T):
    """exp1_sum at +0 (a variable without edges: both exps are 1), below -104.5 (the unclamped branch: +0, beside a finite other side and on
    both sides at once) and at NaN (the 0 / 0 of the hub whose two sums vanish reaches the surveys, then P and N): one, two and eight sweeps"""
    b = _range_batch()
    ref = oracle_forward(oracle, b, T, 0.05, 8)
    res = ref[1]
    it = res['iterations_run']
    assert it == T
    deg = np.bincount(b['graph_map'][0], minlength=b['batch_variable_map'].size)
    assert (deg == 0).sum() >= 5
    sums = [row_sums(b, res, s) for s in range(it)]
    assert any((((P < -104.5) & (N > -50.0)) | ((N < -104.5) & (P > -50.0))).any() for P, N in sums)      # exp(opp) == +0 beside a finite other side
    assert any(((P < -104.5) & (N < -104.5)).any() for P, N in sums)
    if T >= 8:
        # a NaN survey entered a compared sweep's row sums: P and N of its variable are NaN together from then on
        nan_eta = [s for s in range(it) if np.isnan(res['trace_fs'][s][:, 0]).any()]
        assert nan_eta and nan_eta[0] + 1 < it
    solve_and_compare(oracle, b, T, 0.05, 8, ref=ref)


# ---- workgroup sizes, the large image, the isolated form ---------------------------------------------------------------------------------
@pytest.mark.parametrize('threads', ['256', '512', '1024'])
def test_thread_counts(oracle, monkeypatch, threads):
    "variable-row items per wave, helper waves and the cached P4 item all depend on the workgroup size; the per-variable exps must not"
    monkeypatch.setenv('PDP_SOLVE_LDS_THREADS', threads)
    b = random_batch(**DECIMATING)
    solve_and_compare(oracle, b, 60, 0.05, 8)
    b = random_batch(batch=6, n=200, k=3, seed=11)
    solve_and_compare(oracle, b, 30, 0.02, 100)


def test_instance_past_80_kb(oracle):
    "a rung of the 4.2 ladder whose image is past 80 KiB: one workgroup per CU, 1 024 threads, four variable-row items on sixteen waves"
    name = next(nm for nm in families.NAMES if nm.startswith('ladder-4.2') and
                (lambda L: L is not None and L['threads'] == 1024 and L['image'] > 80 * 1024)(families.solver_launch(families.table(families.batch(nm)))) and
                all(families.fits_lds(r) for r in families.table(families.batch(nm))))
    b = families.batch(name)
    solve_and_compare(oracle, b, 40, 0.05, 8)


def test_isolated_one_launch_form(oracle):
    """--isolated: no batch-wide couplings, the whole loop in one launch; without a NaN in the batch the result is the strict mode's, i.e. the
    oracle's"""
    b = random_batch(**DECIMATING)
    ref = oracle_forward(oracle, b, 80, 0.05, 8)
    assert not np.isnan(ref[1]['fs']).any()
    solve_and_compare(oracle, b, 80, 0.05, 8, ref=ref, isolated=True)


# ---- the instantiations that keep their four exps share the file and the carve ------------------------------------------------------------
def test_forced_and_reinforce_forward_unchanged(oracle):
    from test_hip_solve import _reinforce_pair
    from pdp import native
    res = _reinforce_pair(oracle, random_batch(batch=32, n=50, k=3, seed=70), 40, 0.1, 0.5, 70)
    assert np.abs(res['fs'][:, 1]).sum() > 0
    # the SP triple with a caller's force column (k_sp_solve_lds<true, false, false, *>) against the oracle's loop of step-wise operators
    pi, T, tol, t_max = 0.1, 50, 0.05, 8
    b = random_batch(batch=200, n=30, k=3, m=100, seed=300)
    hp, op = make_pair(oracle, b)
    hp.simplify(); op.simplify()
    E, B = op.E, op.B
    q = np.full((E, 3), 1.0 / 3.0, np.float32)
    fs = np.zeros((E, 2), np.float32); fs[:, 0] = 0.5
    fs[:, 1] = np.random.RandomState(3).choice([-1.0, 0.0, 1.0], size=E).astype(np.float32)
    hq, hfs = t(q), t(fs)
    ham = torch.ones(B, dtype=torch.uint8, device='cuda:0')
    iters, used_lds = hp.sp_solve(hq, hfs, ham, native.Decimator(hp), T, tol, t_max, pi=pi)
    assert used_lds and native.kernel_name('sp_solve').startswith('k_sp_solve_lds<true, false, false')
    oam = np.ones(B, np.uint8)
    od = op.new_decimator()
    use_mask, it = False, 0
    for _ in range(T):
        em = op.refresh_edge_mask()[0] if use_mask else None
        q, fs = op.sp_propagate(q, fs, em, oam, q, fs, pi)
        oam, _n = op.sequential_decimate(od, fs, oam, tol, t_max, pi)
        _, s_ = op.refresh_edge_mask()
        use_mask = use_mask or s_ < E
        oam = op.check_termination(oam, op.update_solution(op.state()[2]))
        it += 1
        if int(oam.sum()) <= 0:
            break
    op.free_decimator(od)
    assert iters == it and (op.state()[0] == 0).sum() > 0
    np.testing.assert_array_equal(npy(ham), oam)
    np.testing.assert_array_equal(npy(hp.active_variables)[:, 0], op.state()[0])
    np.testing.assert_array_equal(npy(hp.solution), op.state()[2])
    np.testing.assert_array_equal(npy(hq), q)
    np.testing.assert_array_equal(npy(hfs), fs)
