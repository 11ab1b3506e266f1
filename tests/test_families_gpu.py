"""Every structure-dependent kernel on the structured instance families of tests/families.py (hubs, long clauses, sparse regular graphs,
power-law degrees, community structure, size ladders across the routing limits, long unit / pure-literal chains, minimal shapes) against
the CPU oracle.  Every comparison is np.testing.assert_array_equal: bit-exact floats, and NaN positions included -- assert_array_equal
treats NaNs at the same position as equal (the equal_nan semantics tools/parity_soak.py asks np.array_equal for), and a NaN on one side
only is a mismatch.  No tolerance anywhere.  tests/test_families_host.py checks on the oracle alone that these comparisons are not vacuous.

No call here may fail its speculation (batches of 4 to 64 instances never do): the harnesses assert it instead of skipping."""
import numpy as np
import pytest
import torch

import families
from helpers import random_batch
from test_hip_ops import t, npy, make_pair, assert_state_equal
from test_hip_neural import rand_agg, dev_agg
from test_exact_host import dpll, pigeonhole
from test_exact_gpu import planted, satisfies, solve

pytestmark = pytest.mark.gpu

# (hub d >= 1 000 and power law beta 0.9 are NaN-poisoned by the oracle's first sweep: pdp_sp_solve is compared on them for the NaN pattern
#  and the integer state only -- which is what assert_array_equal on a poisoned run amounts to -- and the single-sweep and integer-state
#  operators of test_row_kernels / test_state_kernels cover their arithmetic.)
POISONED_IN_SWEEP_1 = families.POISONED_IN_SWEEP_1
assert POISONED_IN_SWEEP_1 == ['hub-1000', 'hub-3000', 'power-0.9']

_BATCH = {}


def fam(name):
    if name not in _BATCH:
        _BATCH[name] = families.batch(name) if name != 'headline' else random_batch(batch=6, n=200, k=3, m=840, seed=11)
    return _BATCH[name]


def ids(names):
    return [pytest.param(nm, id=nm) for nm in names]


# ---- state kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['default', 'hbm'])
@pytest.mark.parametrize('name', ids(families.NAMES))
def test_state_kernels(oracle, monkeypatch, name, route):
    "simplify (LDS-resident where the batch allows it, and the HBM form), set_variables, the edge mask, the evaluators and the energies"
    if route == 'hbm':
        monkeypatch.setenv('PDP_SIMPLIFY_HBM', '1')
    hp, op = make_pair(oracle, fam(name))
    assert (hp.E, hp.V, hp.F, hp.B) == (op.E, op.V, op.F, op.B)
    hp.simplify(); op.simplify()
    assert_state_equal(hp, op)
    rng = np.random.RandomState(5)
    assign = np.zeros(op.V, np.float32)
    pick = rng.choice(op.V, size=max(1, op.V // 10), replace=False)
    assign[pick] = rng.randint(0, 2, size=len(pick)) * 2 - 1
    ta = t(assign)
    hp.set_variables(ta); a2 = op.set_variables(assign)
    assert_state_equal(hp, op)
    np.testing.assert_array_equal(npy(ta), a2)
    hp.simplify(); op.simplify()                      # a second fix-point from a state that is not the fresh one
    assert_state_equal(hp, op)
    all_active = hp.refresh_edge_mask()
    m, s = op.refresh_edge_mask()
    np.testing.assert_array_equal(npy(hp.edge_mask)[:, 0], m)
    assert all_active == (s == op.E)
    V, B = op.V, op.B
    pred = rng.rand(V).astype(np.float32); pred[rng.rand(V) < 0.3] = 0.5; pred[rng.rand(V) < 0.2] = 1; pred[rng.rand(V) < 0.2] = 0
    hs, hu = hp.cnf_eval(t(pred)); os_, ou = op.cnf_eval(pred)
    np.testing.assert_array_equal(npy(hs)[:, 0], os_); np.testing.assert_array_equal(npy(hu)[:, 0], ou)
    np.testing.assert_array_equal(npy(hp.update_solution(t(pred)))[:, 0], op.update_solution(pred))
    assert_state_equal(hp, op)
    ham = t(np.ones(B, np.uint8)); hp.check_termination(ham, t(pred))
    np.testing.assert_array_equal(npy(ham), op.check_termination(np.ones(B, np.uint8), pred))
    av = op.state()[0]
    a = ((rng.randint(0, 2, size=V) * 2 - 1) * av).astype(np.float32)
    he, hu = hp.energy(t(a)); oe, ou = op.energy(a)
    np.testing.assert_array_equal(npy(he)[:, 0], oe); np.testing.assert_array_equal(npy(hu)[:, 0], ou)
    np.testing.assert_array_equal(npy(hp.energy_diff(t(a)))[:, 0], op.energy_diff(a))
    for p_, coeff, sharp in ((rng.rand(V).astype(np.float32), 1.0, 1), ((rng.rand(V) > 0.5).astype(np.float32), 3.5, 3),
                             ((0.5 + 0.2 * rng.randn(V)).astype(np.float32), 10.0, 5)):
        ref = np.float32(op.sat_loss(p_, np.float32(coeff), 1e-8, sharp))
        got = npy(hp.sat_loss(t(p_), float(np.float32(coeff)), 1e-8, sharp))[0]
        assert (np.isinf(ref) and np.isinf(got)) or (np.isnan(ref) and np.isnan(got)) or ref == got, (ref, got)


# ---- row kernels from random states ------------------------------------------------------------------------------------------------------
def _prepared(oracle, name, seed=0):
    hp, op = make_pair(oracle, fam(name))
    hp.simplify(); op.simplify()
    rng = np.random.RandomState(seed)
    assign = np.zeros(op.V, np.float32)
    pick = rng.choice(op.V, size=max(1, op.V // 8), replace=False)
    assign[pick] = rng.randint(0, 2, size=len(pick)) * 2 - 1
    hp.set_variables(t(assign)); op.set_variables(assign)
    hp.refresh_edge_mask(); op.refresh_edge_mask()
    return hp, op, rng


@pytest.mark.parametrize('name', ids(families.NAMES))
def test_row_kernels(oracle, monkeypatch, name):
    """smooth_max, instance_max / argmax, one SP sweep (fused and in three phases, with and without the masks, pi 0 and 0.1), the survey
    scorer, and three sequential-decimator steps -- from random states, so that a hub row or a long clause carries non-trivial values"""
    from pdp import native
    hp, op, rng = _prepared(oracle, name)
    E, V, B = op.E, op.V, op.B
    x = rng.rand(E).astype(np.float32); x[rng.rand(E) < 0.1] = 0
    np.testing.assert_array_equal(npy(hp.smooth_max(t(x)))[:, 0], op.smooth_max(x))
    for xv in (rng.rand(V) * (rng.rand(V) > 0.2), rng.randn(V), np.round(rng.randn(V) * 3)):
        xv = xv.astype(np.float32)
        np.testing.assert_array_equal(npy(hp.instance_max(t(xv))), op.instance_max(xv))
        np.testing.assert_array_equal(npy(hp.instance_argmax(t(xv))), op.instance_argmax(xv))
    em, _ = op.refresh_edge_mask()
    for pi in (0.0, 0.1):
        q = rng.rand(E, 3).astype(np.float32); q /= q.sum(1, keepdims=True); q[rng.rand(E) < 0.05, 0] = 0
        fs = rng.rand(E, 2).astype(np.float32); fs[rng.rand(E) < 0.05, 0] = 1.0
        fs[:, 1] = rng.randint(-1, 2, size=E) if pi > 0 else 0
        iq = rng.rand(E, 3).astype(np.float32); ifs = rng.rand(E, 2).astype(np.float32)
        am = (rng.rand(B) > 0.3).astype(np.uint8)
        for fused in (False, True):
            if fused:
                monkeypatch.setenv('PDP_SP_SWEEP_FUSED', '1')
            else:
                monkeypatch.delenv('PDP_SP_SWEEP_FUSED', raising=False)
            for use_mask in (True, False):
                hq, hfs = hp.sp_propagate(t(q), t(fs), hp.edge_mask if use_mask else None, t(am) if use_mask else None, t(iq), t(ifs), pi)
                oq, ofs = op.sp_propagate(q, fs, em if use_mask else None, am if use_mask else None, iq, ifs, pi)
                np.testing.assert_array_equal(npy(hq), oq, err_msg='q fused=%s mask=%s pi=%g' % (fused, use_mask, pi))
                np.testing.assert_array_equal(npy(hfs), ofs, err_msg='fs fused=%s mask=%s pi=%g' % (fused, use_mask, pi))
        monkeypatch.delenv('PDP_SP_SWEEP_FUSED', raising=False)
        np.testing.assert_array_equal(npy(hp.survey_score(t(fs), pi))[:, 0], op.survey_score(fs, pi))
    # three consecutive decimator steps on a fresh pair (the loop of test_sequential_decimator_steps)
    hp, op = make_pair(oracle, fam(name))
    hp.simplify(); op.simplify()
    q = np.full((E, 3), 1.0 / 3.0, np.float32); fs = np.zeros((E, 2), np.float32); fs[:, 0] = 0.5
    hq, hfs = t(q), t(fs)
    ham = t(np.ones(B, np.uint8)); oam = np.ones(B, np.uint8)
    hd = native.Decimator(hp); od = op.new_decimator()
    use_mask = False
    for it in range(3):
        hq, hfs = hp.sp_propagate(hq, hfs, hp.edge_mask if use_mask else None, ham, hq, hfs, 0.0)
        q, fs = op.sp_propagate(q, fs, op.refresh_edge_mask()[0] if use_mask else None, oam, q, fs, 0.0)
        np.testing.assert_array_equal(npy(hq), q, err_msg='q it %d' % it)
        np.testing.assert_array_equal(npy(hfs), fs, err_msg='fs it %d' % it)
        # (a huge tolerance: the decimation fires in every step, also on surveys that have not converged)
        hp.sequential_decimate(hd, hfs, ham, 10.0, 0, 0.0)
        oam, _ = op.sequential_decimate(od, fs, oam, 10.0, 0, 0.0)
        np.testing.assert_array_equal(npy(ham), oam, err_msg='active mask it %d' % it)
        assert_state_equal(hp, op)
        all_active = hp.refresh_edge_mask()
        m, s = op.refresh_edge_mask()
        np.testing.assert_array_equal(npy(hp.edge_mask)[:, 0], m)
        assert all_active == (s == E)
        use_mask = use_mask or not all_active
    op.free_decimator(od)


@pytest.mark.parametrize('name', ids(families.NAMES))
def test_stepwise_reinforce_kernels(oracle, name):
    """reinforce_decimate / reinforce_predict through the step-wise loop (the statements of solver.py:355-386 with the Reinforce triple)
    against the oracle's Reinforce forward on the same coins: end state bit for bit"""
    from pdp import native
    T, pi, dprob = 6, 0.1, 0.5
    hp, op = make_pair(oracle, fam(name))
    coins = np.random.RandomState(3).rand(T).astype(np.float32)
    res = op.forward('reinforce', T, local_search_iterations=0, pi=pi, decimation_probability=dprob, stream=coins, trace=True)
    hp.simplify()
    E, B = hp.E, hp.B
    q = torch.full((E, 3), 1.0, device='cuda:0') / 3.0
    fs = torch.zeros(E, 2, device='cuda:0'); fs[:, 0] = 0.5
    am = torch.ones(B, dtype=torch.uint8, device='cuda:0')
    dec = native.Decimator(hp)
    use_mask, it = False, 0
    for i in range(T):
        q, fs = hp.sp_propagate(q, fs, hp.edge_mask if use_mask else None, am, q, fs, pi)
        hp.reinforce_decimate(dec, fs, am, float(coins[i]), dprob, pi)
        use_mask = use_mask or not hp.refresh_edge_mask()
        pred = hp.update_solution(hp.reinforce_predict(fs).reshape(-1).contiguous())
        hp.check_termination(am, pred.reshape(-1).contiguous())
        it += 1
        if int(am.sum().item()) <= 0:
            break
    assert it == res['iterations_run']
    np.testing.assert_array_equal(npy(am), res['trace_active_mask'][it - 1])
    np.testing.assert_array_equal(npy(hp.solution), res['trace_solution'][it - 1])
    np.testing.assert_array_equal(npy(q), res['q'])
    np.testing.assert_array_equal(npy(fs), res['fs'])


# ---- pdp_sp_solve ----------------------------------------------------------------------------------------------------------------------------
ROUTES = {'resident': {}, 'hbm': {'PDP_SOLVE_FORCE_HBM': '1'}, 'lockstep': {'PDP_SOLVE_FORCE_LOCKSTEP': '1'}, 'chunk7': {'PDP_SOLVE_CHUNK': '7'}}
_ORACLE = {}
COINS = np.random.RandomState(1).rand(40).astype(np.float32)


def oracle_run(oracle, name, model, T, trace_float=False):
    "the oracle's loop on a fresh problem; kept per (batch, model, T): the four routes compare against the same run"
    key = (name, model, T)
    if key in _ORACLE and not trace_float:
        return _ORACLE[key]
    b = fam(name)
    op = oracle.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], 1)
    if model == 'sp':
        res = op.forward('p-d-p', T, local_search_iterations=0, tolerance=0.05, t_max=8, seed=5, trace=True, trace_float=trace_float)
    else:
        res = op.forward('reinforce', T, local_search_iterations=0, pi=0.1, decimation_probability=0.5, stream=COINS[:T], trace=True, trace_float=trace_float)
    if trace_float:
        return res
    it = res['iterations_run']
    _ORACLE[key] = dict(it=it, q=res['q'], fs=res['fs'], rand=res['rand_consumed'],
                        **{k: res['trace_' + k][it - 1].copy() for k in ('active_mask', 'active_var', 'active_fn', 'solution')})
    return _ORACLE[key]


_PLAN = {}


def plan(oracle, name, model):
    "sweep counts of the compared runs: 40, and the last NaN-free count where the oracle poisons the batch later than its first sweep"
    if (name, model) not in _PLAN:
        _PLAN[(name, model)] = families.sweep_plan(lambda T: oracle_run(oracle, name, model, T, trace_float=True))
    return _PLAN[(name, model)]


def solve_and_compare(oracle, name, model, T, expect=None):
    from pdp import native
    ref = oracle_run(oracle, name, model, T)
    b = fam(name)
    hp = native.Problem(t(b['graph_map']), t(b['batch_variable_map']), t(b['batch_function_map']), t(b['edge_feature']))
    hp.simplify()
    E, B = hp.E, hp.B
    q = torch.full((E, 3), 1.0, device='cuda:0') / 3.0
    fs = torch.zeros(E, 2, device='cuda:0'); fs[:, 0] = 0.5
    am = torch.ones(B, dtype=torch.uint8, device='cuda:0')
    dec = native.Decimator(hp)
    try:
        if model == 'sp':
            iters, used_lds = hp.sp_solve(q, fs, am, dec, T, 0.05, 8)
        else:
            iters, used_lds = hp.sp_solve(q, fs, am, dec, T, 0.01, 0.0, pi=0.1, model=native.MODEL_REINFORCE, coins=t(COINS[:T]), decimation_probability=0.5)
        spec_ok = True
    except native.SpeculationFailed:
        spec_ok = False
    assert spec_ok, "a batch of 4 to 64 instances never fails its speculation"
    assert iters == ref['it']
    if model == 'rf':
        assert ref['rand'] == ref['it']
    np.testing.assert_array_equal(npy(am), ref['active_mask'])
    np.testing.assert_array_equal(npy(hp.active_variables)[:, 0], ref['active_var'])
    np.testing.assert_array_equal(npy(hp.active_functions)[:, 0], ref['active_fn'])
    np.testing.assert_array_equal(npy(hp.solution), ref['solution'])
    np.testing.assert_array_equal(npy(q), ref['q'])
    np.testing.assert_array_equal(npy(fs), ref['fs'])
    if expect is not None:
        # (a resident run whose speculation failed is rolled back and served by the lock-step launch: used_lds is False then)
        assert (used_lds, hp.last_solve_stats['hbm_instances']) == expect, (used_lds, hp.last_solve_stats)
    return ref


def expected_route(name, route):
    "(used_lds, hbm_instances) the family is meant to reach on a route"
    fits = [families.fits_lds(r) for r in families.table(fam(name))]
    B, big = len(fits), len(fits) - sum(fits)
    if route in ('hbm', 'lockstep') or big == B:
        return (False, B)
    return (True, big)


@pytest.mark.parametrize('model', ['sp', 'rf'])
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('name', ids(families.NAMES))
def test_sp_solve(oracle, monkeypatch, name, route, model):
    """p-d-p and Reinforce in one persistent call on the resident route, the HBM-resident kernel, the lock-step launch and a short chunk
    schedule: the full end state of test_persistent_solve_matches_oracle_loop (active_functions included), the route the family is meant
    to reach (the ladders across the LDS limit and the big hub report both kinds of instance in one call), for 40 sweeps and -- where the
    oracle poisons the batch on the way -- also for the NaN-free sweeps before the poison."""
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    expect = expected_route(name, route)
    nan_seen = False
    for T in plan(oracle, name, model):
        ref = solve_and_compare(oracle, name, model, T, expect)
        nan_seen = nan_seen or bool(np.isnan(ref['fs']).any() or np.isnan(ref['q']).any())
    if len(plan(oracle, name, model)) > 1 or name in POISONED_IN_SWEEP_1:
        assert nan_seen
    if families.promise(name).get('mixed_routes') and route in ('resident', 'chunk7'):
        assert expect[0] and 0 < expect[1] < len(families.table(fam(name)))


def test_ladders_report_both_kinds_in_one_call():
    "what test_sp_solve expects of the ladder batches that straddle the LDS limit: LDS-resident and HBM-resident instances in one call"
    seen = [nm for nm in families.NAMES if nm.startswith('ladder') and expected_route(nm, 'resident')[0] and expected_route(nm, 'resident')[1] > 0]
    assert any(nm.startswith('ladder-4.2') for nm in seen) and any(nm.startswith('ladder-3.0') for nm in seen)


@pytest.mark.parametrize('model', ['sp', 'rf'])
@pytest.mark.parametrize('threads', ['256', '512', '1024'])
@pytest.mark.parametrize('name', ['headline', 'regular-4-3-n600', 'hub-254-255-256-257'])
def test_sp_solve_thread_count_invariance(oracle, monkeypatch, name, threads, model):
    """The LDS-resident solver under each thread count the library itself chooses (256 / 512 / 1 024): 256 threads on the headline shape
    (n = 200, m = 840) is the uncached work-item form without helper waves on a dense instance; every run equals the oracle."""
    monkeypatch.setenv('PDP_SOLVE_LDS_THREADS', threads)
    for T in plan(oracle, name, model):
        solve_and_compare(oracle, name, model, T, (True, 0))


# ---- Walk-SAT ----------------------------------------------------------------------------------------------------------------------------------
def _walksat(oracle, name, mode, w):
    hp, op = make_pair(oracle, fam(name))
    hp.simplify(); op.simplify()
    rng = np.random.RandomState(7)
    n_active = int((op.state()[0] > 0).sum())
    if mode == 'stream':
        stream = rng.rand(n_active + w * (op.V + op.B)).astype(np.float32)
        hp.random_fill(values=t(stream[:n_active]) if n_active else t(np.zeros(1, np.float32)))
        cur = op.random_fill(stream=stream)
        assert cur == n_active
        assert_state_equal(hp, op)
        rest = stream[n_active:].reshape(w, op.V + op.B)
        var_rand = np.ascontiguousarray(rest[:, :op.V]); coin = np.ascontiguousarray(rest[:, op.V:])
        pred = op.state()[2]
        hout, hsteps = hp.local_search(t(pred), w, 0.5, t(var_rand), t(coin))
        oout, osteps, cur2 = op.local_search(pred, w, 0.5, stream=stream, cursor=cur)
        assert cur2 == n_active + osteps * (op.V + op.B)
    else:
        hp.random_fill(seed=1234); op.random_fill(seed=1234)
        assert_state_equal(hp, op)
        pred = op.state()[2]
        hout, hsteps = hp.local_search(t(pred), w, 0.5, seed=99)
        oout, osteps, _ = op.local_search(pred, w, 0.5, seed=99)
    assert hsteps == osteps
    np.testing.assert_array_equal(npy(hout)[:, 0], oout)


BIG_WALKSAT = ['hub-3000', 'long-1000', 'chains-4000', 'ladder-4.2-n340-420', 'ladder-4.2-n620-700', 'ladder-3.0-n500-580', 'regular-6-3-n800']


@pytest.mark.parametrize('form', ['persistent', 'strict'])
@pytest.mark.parametrize('name', ids(families.NAMES))
def test_walksat(oracle, monkeypatch, name, form):
    "random_fill + local_search with stream and Philox numbers, 5 and 200 steps: the persistent kernels (routed per instance) and the strict loop"
    if form == 'strict':
        monkeypatch.setenv('PDP_WALKSAT_STRICT', '1')
    for mode in ('stream', 'philox'):
        for w in (5, 200):
            _walksat(oracle, name, mode, w)


@pytest.mark.parametrize('name', ids(BIG_WALKSAT))
def test_walksat_big_instances_on_one_workgroup(oracle, monkeypatch, name):
    "the batches with instances past Walk-SAT's 64 KiB LDS limit: PDP_WALKSAT_NO_TEAM next to the team form test_walksat runs"
    assert any(families.walksat_lds_bytes(r['n'], r['m'], r['e']) > 64 * 1024 for r in families.table(fam(name)))
    monkeypatch.setenv('PDP_WALKSAT_NO_TEAM', '1')
    for mode in ('stream', 'philox'):
        _walksat(oracle, name, mode, 200)


@pytest.mark.parametrize('threads', ['64', '128', '256'])
@pytest.mark.parametrize('name', ['headline', 'regular-4-3-n600', 'hub-254-255-256-257'])
def test_walksat_thread_count_invariance(oracle, monkeypatch, name, threads):
    monkeypatch.setenv('PDP_WALKSAT_THREADS', threads)
    for mode in ('stream', 'philox'):
        _walksat(oracle, name, mode, 200)


# ---- neural operators ------------------------------------------------------------------------------------------------------------------------
def ordered_row_sum(rows, nrows, x):
    "float32 sum of x [E, A] over the edges of every row in ascending edge order, one addition after the other"
    order = np.argsort(rows, kind='stable')
    ptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=nrows))]
    deg = np.diff(ptr)
    acc = np.zeros((nrows, x.shape[1]), np.float32)
    for j in range(int(deg.max())):
        sel = np.nonzero(deg > j)[0]
        acc[sel] = acc[sel] + x[order[ptr[sel] + j]]
    return acc


@pytest.mark.parametrize('H,m1,a,g', [(128, 100, 50, 100), (20, 36, 17, 40)])
@pytest.mark.parametrize('name', ids(['hub-1000', 'long-257', 'regular-4-3-n1000', 'minimal']))
def test_neural_operators(oracle, name, H, m1, a, g):
    """one aggregator call by variable and by clause, one GRU, one predictor, and the training path's ordered row sums, on a hub of 1 000
    edges, a clause of 257 literals, 4 000 rows of degree 4 and the minimal shapes: hidden 128 (the MFMA kernels) and a generic width"""
    from pdp import native
    from pdp.nn import train_ops
    hp, op, rng = _prepared(oracle, name, seed=H)
    em, _ = op.refresh_edge_mask()
    ev, ec, es, vi, fi = op.graph()
    E, V, F, B = op.E, op.V, op.F, op.B
    state = (rng.randn(E, H) * 0.5).astype(np.float32); old = (rng.randn(E, H) * 0.5).astype(np.float32)
    am = (rng.rand(B) > 0.3).astype(np.uint8)
    mask = am[vi[ev]].astype(np.float32)
    w = rand_agg(rng, H + 1, m1, a, g, H, 1)
    for by_var, rows, nrows in ((True, ev, V), (False, ec, F)):
        ref = oracle.aggregator(rows, nrows, state, es, em, False, w)
        ref = mask[:, None] * ref + (1.0 - mask[:, None]) * old
        got = hp.neural_aggregate_edges(dev_agg(w, 1), by_var, t(state), hp.edge_mask, t(am), t(old))
        np.testing.assert_array_equal(npy(got), ref.astype(np.float32), err_msg='aggregator by_var=%s' % by_var)
    s = lambda *sh: (rng.randn(*sh) * 0.2).astype(np.float32)  # noqa: E731
    gw = dict(W_ih=s(3 * H, H + 1), W_hh=s(3 * H, H), b_ih=s(3 * H), b_hh=s(3 * H))
    hprev = (rng.randn(E, H) * 0.5).astype(np.float32)
    ref = oracle.gru(state, es, hprev, mask=mask, **gw)
    got = hp.neural_gru(native.GruWeights(t(gw['W_ih']), t(gw['W_hh']), t(gw['b_ih']), t(gw['b_hh'])), t(state), t(hprev), t(am))
    np.testing.assert_array_equal(npy(got), ref)
    wp = rand_agg(rng, H + 1, m1, a, g, H, 0)
    hw = dict(W1=s(50, H), b1=s(50), W2=s(1, 50))
    agg = oracle.aggregator(ev, V, state, es, em, True, wp)
    ref = oracle.perceptron(agg, hw['W1'], hw['b1'], hw['W2'])
    got = hp.neural_predict(dev_agg(wp, 0), native.HeadWeights(t(hw['W1']), t(hw['b1']), t(hw['W2']), 'sigmoid'), t(state), hp.edge_mask)
    np.testing.assert_array_equal(npy(got), ref)
    # train_row_sum / train_row_spread: an even width (two columns per thread) and an odd one
    for A in (a, a + 1):
        x = (rng.randn(E, A) * 0.5).astype(np.float32)
        for by_var, rows, nrows in ((True, ev, V), (False, ec, F)):
            want = ordered_row_sum(rows, nrows, x)
            with torch.no_grad():
                got_rows = train_ops.RowAggregate.apply(t(x), hp, by_var, True)
                got_edges = train_ops.RowAggregate.apply(t(x), hp, by_var, False)
            np.testing.assert_array_equal(npy(got_rows), want, err_msg='row sum A=%d by_var=%s' % (A, by_var))
            np.testing.assert_array_equal(npy(got_edges), want[rows] - x, err_msg='row spread A=%d by_var=%s' % (A, by_var))


# ---- complete solver ---------------------------------------------------------------------------------------------------------------------------
def test_exact_solver_on_family_instances():
    "status = the reference DPLL's answer on hub, long-clause, regular, power-law, minimal and small threshold instances; models hold"
    cases = families.exact_cases()
    inst = [(n, c) for _, n, c in cases]
    want = np.array([dpll(n, c) for n, c in inst])
    assert want.sum() >= 5 and (~want).sum() >= 5
    status, models, _ = solve(inst)
    np.testing.assert_array_equal(status == 1, want)
    assert set(np.unique(status)) <= {0, 1}
    for (name, n, c), s_, m in zip(cases, status, models):
        assert not s_ or satisfies(c, m), name


def _cores():
    "pigeonhole 5 and 6 and one threshold 3-SAT instance of each answer, with the reference DPLL's answer on the core alone"
    thr = [(c, dpll(*c)) for c in families.threshold_cores()]
    sat, unsat = next(c for c, w in thr if w), next(c for c, w in thr if not w)
    return [('php5', pigeonhole(5), False), ('php6', pigeonhole(6), False), ('threshold-sat', sat, True), ('threshold-unsat', unsat, False)]


def test_exact_solver_backtracks_on_the_hbm_route():
    """The disjoint union of a planted alpha-2 instance on 20 000 variables (60 000 literals: the HBM-resident form) and a small hard core
    on its own variables -- pigeonhole 5 and 6, threshold 3-SAT with both answers -- with the core first, last and interleaved: the
    union's status is the core's (reference DPLL on the core alone), a model satisfies every clause, and status / model / work are the
    same with the union alone in its batch and among small instances (the header's promise: deterministic and instance-local).
    The same unions with a planted part of 1 000 variables fit the 48 KiB LDS slab.  The header promises nothing about the values of
    the core's variables across two DIFFERENT unions, so between the two routes only status and model validity are compared.
    (All placements share one batch: a satisfiable union costs the HBM-resident search some 20 s, whatever its core.)"""
    from test_exact_gpu import random_instance
    cores = _cores()
    assert {w for _, _, w in cores} == {True, False}
    rng = np.random.RandomState(4)
    small = [random_instance(rng, 12) for _ in range(20)]
    for seed, big_n in ((10, 1000), (9, 20000)):
        big = planted(big_n, 2.0, 3, seed)
        cases = [(name, place, want) + families.compose(core, big, place)[:2] for place in ('first', 'last', 'interleaved') for name, core, want in cores]
        inst = [(n, c) for _, _, _, n, c in cases]
        for n, c in inst:
            slab = 25 * n + 2 * sum(len(x) for x in c) + 2 * len(c) + 64              # (ex_lds_layout of csrc/pdp_exact.hip)
            assert (slab <= 48 * 1024) == (big_n == 1000)
        mixed = small[:10] + inst[:5] + small[10:] + inst[5:]
        status, models, work = solve(mixed)
        pos = list(range(10, 15)) + list(range(25, 25 + len(inst) - 5))
        for (name, place, want, n, c), i in zip(cases, pos):
            tag = (name, place, big_n)
            assert status[i] == (1 if want else 0), tag
            if want:
                assert satisfies(c, models[i]), tag
            else:
                assert not models[i].any(), tag
            s1, m1, w1 = solve([(n, c)])
            assert s1[0] == status[i] and w1[0] == work[i] and np.array_equal(m1[0], models[i]), tag
