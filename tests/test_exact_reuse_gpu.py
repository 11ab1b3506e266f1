"""Slab reuse and relaunch of the complete solvers on the GPU.  The persistent kernels of csrc/pdp_exact.hip (k_exact<HINT>,
k_exact_learn<HINT, PROOF>, k_exact_check) launch min(B, CUs * resident workgroups) waves that take instance after instance from one
counter; a batch smaller than that product -- every batch of the other exact modules on an MI355X -- gives each wave one instance, so
nothing there runs an instance in the slab, or in the HBM arrays of a handle, that another one left.  Here PDP_EXACT_GRID lowers the grid
to 1, 2 or 3 waves (read back with Problem.exact_last_grid() after every launch, so that a dead switch cannot turn these into the tests
that exist already), one batch is larger than twice the natural grid, and one handle is launched eleven times.  Every comparison is
equality with the Python models (tests/exact_model.py, exact_learn_model.py, exact_proof_model.py) on the batches of tests/exact_reuse.py,
whose properties test_exact_reuse_host.py asserts."""
import numpy as np
import pytest
import torch

import exact_proof_model as pm
import exact_reuse as xr
import exact_wide as xw
from test_exact_learn_gpu import on_lds, problem, same, split
from test_exact_proof_gpu import CHECK_PAD_N, SENTINEL, check_cases, check_on_lds, run_check, run_proof, same_check, same_search, untouched
from test_exact_wide_gpu import KINDS, LEARN_BATCHES, hints_for, leading, padded, plain_on_lds, same_plain

pytestmark = pytest.mark.gpu


def switch(monkeypatch, v):
    "PDP_EXACT_GRID=v for the launches that follow; None: unset, the natural grid"
    if v is None:
        monkeypatch.delenv('PDP_EXACT_GRID', raising=False)
    else:
        monkeypatch.setenv('PDP_EXACT_GRID', str(v))


def launched(p, v):
    """the last launch on p used the grid the switch asks for; None: the natural grid min(B, CUs * resident workgroups), which is B for the
    batches this is used on (at most a few hundred instances; the product is in the thousands, test_natural_grid)"""
    g = p.exact_last_grid()
    assert g == (p.B if v is None else min(v, p.B)), (g, v, p.B)
    return g


def hint_tensor(p, hints):
    return None if hints is None else torch.from_numpy(np.concatenate([np.asarray(h, dtype=np.float32) for h in hints])).to(p.device)


def search(p, inst, v, hints=None, budget=0, arena=0, learn=True):
    "test_exact_learn_gpu.lsolve on a given handle, with the grid of its launch asserted"
    hint = hint_tensor(p, hints)
    if learn:
        st, model, wk, ln = p.exact_solve(budget, hints=hint, learn=True, arena=arena, stats=True)
        launched(p, v)
        ln, red = ln.cpu().numpy(), p.exact_learn_reductions().cpu().numpy()
    else:
        (st, model, wk), ln, red = p.exact_solve(budget, hints=hint), None, None
        launched(p, v)
    return st.cpu().numpy(), split(inst, model.cpu().numpy()), wk.cpu().numpy(), ln, red


def logged(p, inst, v, **kw):
    out = run_proof(inst, prob=p, **kw)
    launched(p, v)
    return out


def checked(p, v, inst, status, models, regions, plen, budget=0):
    out = run_check(inst, status, models, regions, plen, budget, prob=p)
    launched(p, v)
    return out


def test_last_grid_before_the_first_launch():
    p = problem(xr.tiny()[:3])
    assert p.exact_last_grid() == 0


# ---- a. the mixed batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [1, 2, 3])
def test_mixed_batch_under_reuse(monkeypatch, grid):
    "all 473 instances of test_exact_learn_gpu.py: the plain search and the learning search at the three arenas, on one handle"
    inst, runs = xr.mixed()
    switch(monkeypatch, grid)
    p = problem(inst)
    same_plain(search(p, inst, grid, budget=xr.MIXED_BUDGET, learn=False), xr.mixed_plain(None)[0])
    for arena in (0, 12, 40):
        got = search(p, inst, grid, arena=arena)
        same(got, runs[arena])
        assert got[4].any() == (arena != 0) and (arena != 12 or (got[0] == -1).any())      # 40 words are reduced, 12 words also run out


@pytest.mark.parametrize('kind', ['own', 'nan30'])
def test_mixed_batch_hinted_under_reuse(monkeypatch, kind):
    inst, _ = xr.mixed()
    switch(monkeypatch, 1)
    p = problem(inst)
    got = search(p, inst, 1, hints=xr.mixed_hints()[kind], budget=xr.MIXED_BUDGET, learn=False)
    same_plain(got, xr.mixed_plain(kind)[0])


# ---- b. the wide instances with their small neighbours -----------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [1, 2])
@pytest.mark.parametrize('route', ['lds', 'hbm'])
@pytest.mark.parametrize('name', LEARN_BATCHES)
def test_wide_learning_batches_under_reuse(monkeypatch, name, route, grid):
    inst, arena, budget = xw.learn_batches()[name]
    want, _ = xw.learn_results(name)
    batch = inst if route == 'lds' else padded(inst, xw.LEARN_PAD_N)
    assert all(on_lds(i, arena) == (route == 'lds') for i in batch)
    switch(monkeypatch, grid)
    leading(search(problem(batch), batch, grid, budget=budget, arena=arena), want)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('route', ['lds', 'hbm'])
def test_wide_plain_batch_under_reuse(monkeypatch, route, kind):
    inst = xw.plain_batch()
    want, _ = xw.plain_results(kind)
    n = None if route == 'lds' else xw.PLAIN_PAD_N
    batch = inst if route == 'lds' else padded(inst, n)
    assert all(plain_on_lds(i) == (route == 'lds') for i in batch)
    switch(monkeypatch, 1)
    leading(search(problem(batch), batch, 1, hints=hints_for(kind, n), budget=xw.PLAIN_BUDGET, learn=False), want)


# ---- c. crossing() and shrinking() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['crossing', 'shrinking'])
def test_crossing_and_shrinking(monkeypatch, which):
    """one wave, every search, one handle: each successor has fewer literals than its predecessor and (crossing) more variables, so its
    4-byte arrays begin over the predecessor's literals"""
    inst = getattr(xr, which)()
    hints = xr.padded_hints(xr.cross_hints(), inst)
    switch(monkeypatch, 1)
    p = problem(inst)
    leading(search(p, inst, 1, budget=xr.CROSS_BUDGET, learn=False), xr.cross_plain(False)[0])
    leading(search(p, inst, 1, hints=hints, budget=xr.CROSS_BUDGET, learn=False), xr.cross_plain(True)[0])
    for arena in (0, xr.CROSS_ARENA):
        leading(search(p, inst, 1, budget=xr.CROSS_BUDGET, arena=arena), xr.cross_learn(arena)[0])
        leading(search(p, inst, 1, hints=hints, budget=xr.CROSS_BUDGET, arena=arena), xr.cross_learn(arena, True)[0])
        out = logged(p, inst, 1, budget=xr.CROSS_BUDGET, arena=arena)
        same_search(out, xr.cross_proof(arena))
        assert untouched(out) and out['plen'].max() > 8
    if which == 'crossing':
        switch(monkeypatch, 2)
        for arena in (0, xr.CROSS_ARENA):
            leading(search(p, inst, 2, budget=xr.CROSS_BUDGET, arena=arena), xr.cross_learn(arena)[0])


# ---- d. both routes in one batch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [1, None])
def test_routes(monkeypatch, grid):
    "under grid 1 one wave runs the HBM-routed instances in the handle's HBM arrays first and then the LDS-routed ones in its slab"
    inst, _ = xr.routes()
    switch(monkeypatch, grid)
    p = problem(inst)
    leading(search(p, inst, grid, budget=xr.ROUTES_BUDGET, learn=False), xr.routes_plain(None)[0])
    for arena in (0, xr.ROUTES_ARENA):
        leading(search(p, inst, grid, budget=xr.ROUTES_BUDGET, arena=arena), xr.routes_learn(arena)[0])
        out = logged(p, inst, grid, budget=xr.ROUTES_BUDGET, arena=arena)
        same_search(out, xr.routes_proof(arena))
        assert untouched(out)


# ---- e. the checker ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [1, 2])
@pytest.mark.parametrize('pad', [0, CHECK_PAD_N])
def test_checker_under_reuse(monkeypatch, pad, grid):
    "genuine, mutated, forged, incomplete and malformed inputs interleaved: a stale request word or value byte could let a forged proof pass"
    batch, status, models, regions, plen, want = check_cases(pad)
    assert all(check_on_lds(i) != bool(pad) for i in batch)
    switch(monkeypatch, grid)
    got = checked(problem(batch), grid, batch, status, models, regions, plen)
    same_check(got, want)
    assert set(np.unique(got[0])) == {-1, 0, 1}


def test_checker_on_both_routes_under_reuse(monkeypatch):
    "every HBM-routed case and every seventh LDS-routed one in one batch, one wave"
    big, small = check_cases(CHECK_PAD_N), check_cases(0)
    keep = list(range(0, len(small[0]) - 1, 7)) + [len(small[0]) - 1]               # the last one is genuine
    cols = [list(b) + [s[i] for i in keep] for b, s in zip(big[:5], small[:5])]
    want = tuple(np.concatenate([b, s[keep]]) for b, s in zip(big[5], small[5]))
    routes = [check_on_lds(i) for i in cols[0]]
    assert routes.count(False) == len(big[0]) and routes.count(True) == len(keep) >= 40
    switch(monkeypatch, 1)
    got = checked(problem(cols[0]), 1, *cols)
    same_check(got, want)
    assert set(np.unique(got[0])) == {-1, 0, 1}


def test_checker_end_to_end_on_the_device_buffers_under_reuse(monkeypatch):
    "test_checker_accepts_what_the_search_logged_and_refutes_a_wrong_status with one wave for the search and for the check"
    inst, want = pm.base_inputs()
    switch(monkeypatch, 1)
    p = problem(inst)
    out = logged(p, inst, 1)
    same_search(out, want[0])
    dev = p.device
    st, model, _, _, proof, off, plen = p.exact_solve_proof()
    launched(p, 1)
    verdict, fail_at, work = [t.cpu().numpy() for t in p.exact_check(st, model, proof, off, plen)]
    launched(p, 1)
    decided = out['status'] != -1
    assert decided.sum() > 400 and (verdict[decided] == 1).all() and (verdict[~decided] == -1).all() and (fail_at == -1).all()
    regions = [pm.words(x) for x in want[0][5]]
    np.testing.assert_array_equal(work, pm.check_all(inst, want[0][0], want[0][1], regions, want[0][6])[2])
    swapped = np.where(decided, 1 - out['status'], -1).astype(np.int8)
    verdict = p.exact_check(torch.from_numpy(swapped).to(dev), model, proof, off, plen)[0].cpu().numpy()
    launched(p, 1)
    assert (verdict[decided] == 0).all()


# ---- f. one handle, many launches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [None, 1])
@pytest.mark.parametrize('batch', ['routes', 'hbm'])
def test_one_handle_many_launches(monkeypatch, batch, grid):
    """the HBM working arrays are cached on the handle (ex_blob, exl_blob, exc_blob): every launch starts on what the one before left, and
    a new arena size rebuilds the learning search's block"""
    inst = xr.routes()[0 if batch == 'routes' else 1]
    cores = xr.routes_cores()
    own, nan30 = (xr.padded_hints(xr.routes_hints()[k], inst) for k in ('own', 'nan30'))
    A, budget = xr.ROUTES_ARENA, xr.ROUTES_BUDGET
    switch(monkeypatch, grid)
    p = problem(inst)
    plain = xr.routes_plain(None)[0]
    leading(search(p, inst, grid, budget=budget, learn=False), plain)                                                # 1
    leading(search(p, inst, grid, hints=own, budget=budget, learn=False), xr.routes_plain('own')[0])                 # 2
    leading(search(p, inst, grid, hints=nan30, budget=budget, learn=False), xr.routes_plain('nan30')[0])             # 3
    leading(search(p, inst, grid, budget=budget, arena=0), xr.routes_learn(0)[0])                                    # 4
    leading(search(p, inst, grid, budget=budget, arena=A), xr.routes_learn(A)[0])                                    # 5: re-prepares
    leading(search(p, inst, grid, hints=nan30, budget=budget, arena=A), xr.routes_learn(A, 'nan30')[0])              # 6
    want = xr.routes_proof(A)
    first = logged(p, inst, grid, budget=budget, arena=A)                                                            # 7
    same_search(first, want)
    r = p.exact_solve_proof(budget, arena=A, proof_off=torch.zeros(p.B + 1, dtype=torch.int64, device=p.device))     # 8: the sizing call
    launched(p, grid)
    assert r[4] is None
    np.testing.assert_array_equal(r[6].cpu().numpy(), want[6])
    np.testing.assert_array_equal(r[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(r[2].cpu().numpy(), want[2])
    again = logged(p, inst, grid, budget=budget, arena=A, sizes=want[6])                                             # 9: regions that just fit
    same_search(again, want)
    assert untouched(again) and (again['plen'] == again['size']).all() and again['plen'].max() > 20
    regions = [pm.words(x) for x in want[5]]
    expect = pm.check_all(cores, want[0], want[1], regions, want[6])
    got = checked(p, grid, inst, again['status'], again['models'], again['words'], again['plen'])                    # 10
    same_check(got, expect)
    assert (got[0][want[0] != -1] == 1).all() and (got[0][want[0] == -1] == -1).all() and (want[0] == 0).sum() >= 10
    leading(search(p, inst, grid, budget=budget, learn=False), plain)                                                # 11


# ---- g. the natural grid -----------------------------------------------------------------------------------------------------------------
def tiled_problem(B):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    raw = [exact.raw_item(n, c) for n, c in xr.tiny()]
    b = dataset.to_torch(dataset.collate_segment([raw[i] for i in xr.tiled_index(B)]), torch.device('cuda:0'))
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=B)


def tiled_launches(p, idx):
    "the four kernels on tiled(B): kernel -> (grid, outputs that equal the tiny instances' model results, tiled)"
    r = xr.tiny_results()
    flat = lambda models: np.concatenate([models[i] for i in idx])
    grids = {}
    st, model, wk = [t.cpu().numpy() for t in p.exact_solve()]
    grids['plain'] = p.exact_last_grid()
    np.testing.assert_array_equal(st, r['plain'][0][idx])
    np.testing.assert_array_equal(wk, r['plain'][2][idx])
    np.testing.assert_array_equal(model, flat(r['plain'][1]))
    st, model, wk, ln = [t.cpu().numpy() for t in p.exact_solve(learn=True, stats=True)]
    grids['learn'] = p.exact_last_grid()
    want = r['proof']
    for g, w in zip((st, wk, ln, p.exact_learn_reductions().cpu().numpy()), (want[0], want[2], want[3], want[4])):
        np.testing.assert_array_equal(g, w[idx])
    np.testing.assert_array_equal(model, flat(want[1]))
    e = p.instance_edges().cpu().numpy()
    from pdp import native
    buf = torch.full((int(e.sum()) * native.PROOF_WORDS_PER_LITERAL + 7,), SENTINEL, dtype=torch.int32, device=p.device)
    st, model, wk, ln, proof, off, plen = p.exact_solve_proof(proof=buf)
    grids['proof'] = p.exact_last_grid()
    got = (st.cpu().numpy(), wk.cpu().numpy(), ln.cpu().numpy(), p.exact_learn_reductions().cpu().numpy(), plen.cpu().numpy())
    for g, w in zip(got, (want[0], want[2], want[3], want[4], want[6])):
        np.testing.assert_array_equal(g, w[idx])
    np.testing.assert_array_equal(model.cpu().numpy(), flat(want[1]))
    # the whole buffer: every region starts with its instance's lemma words, and every other word still holds the sentinel
    off_h = off.cpu().numpy()
    assert (want[6][idx] <= off_h[1:] - off_h[:-1]).all()
    expect = np.full(buf.numel(), SENTINEL, dtype=np.int32)
    for t, words in enumerate(r['regions']):
        assert len(words) == want[6][t]
        expect[off_h[:-1][idx == t][:, None] + np.arange(len(words))[None, :]] = words
    np.testing.assert_array_equal(proof.cpu().numpy(), expect)
    verdict, fail_at, work = [t.cpu().numpy() for t in p.exact_check(st, model, proof, off, plen)]
    grids['check'] = p.exact_last_grid()
    for g, w in zip((verdict, fail_at, work), r['check']):
        np.testing.assert_array_equal(g, w[idx])
    return grids


def test_natural_grid(monkeypatch):
    """no switch: a batch of more than twice the launch grid, so that every wave of all four kernels takes several instances.  B doubles
    from 20 000 until B >= 2 grid + 1 holds for each kernel on the device at hand; past 160 000 the test fails"""
    switch(monkeypatch, None)
    B = 20000
    while True:
        idx = xr.tiled_index(B)
        p = tiled_problem(B)
        grids = tiled_launches(p, idx)
        print("tiled(%d): natural grids %s" % (B, grids))
        if all(B >= 2 * g + 1 for g in grids.values()):
            break
        del p
        B *= 2
        assert B <= 160000, "no batch up to 160 000 instances is larger than twice the natural grid %s" % grids
    # a switch above the natural grid is clipped to it
    switch(monkeypatch, grids['plain'] + 1000)
    st = p.exact_solve()[0].cpu().numpy()
    assert p.exact_last_grid() == grids['plain']
    np.testing.assert_array_equal(st, xr.tiny_results()['plain'][0][idx])


# ---- h. the switch itself ----------------------------------------------------------------------------------------------------------------
def test_switch_values(monkeypatch):
    "0, negative, non-numeric and empty values leave the grid at its natural value; the results never depend on it"
    inst = xr.shrinking()
    want_plain, want_learn = xr.cross_plain(False)[0], xr.cross_learn(0)[0]
    status, models, work, _, _, lemmas, plen = xr.cross_proof(0)
    regions = [pm.words(x) for x in lemmas]
    want_check = pm.check_all(inst, status, models, regions, plen)
    p = problem(inst)
    switch(monkeypatch, None)
    natural = {}
    for value in (None, '0', '-3', 'abc', '', '2x', str(len(inst) + 7), '4'):
        switch(monkeypatch, value)
        expect = 4 if value == '4' else None
        leading(search(p, inst, expect, budget=xr.CROSS_BUDGET, learn=False), want_plain)
        grids = {'plain': p.exact_last_grid()}
        leading(search(p, inst, expect, budget=xr.CROSS_BUDGET, arena=0), want_learn)
        grids['learn'] = p.exact_last_grid()
        same_check(checked(p, expect, inst, status, models, regions, plen), want_check)
        grids['check'] = p.exact_last_grid()
        if value is None:
            natural = grids
        assert grids == ({k: 4 for k in grids} if value == '4' else natural), value
    assert all(4 < g <= len(inst) for g in natural.values())


# ---- i. the fast build -------------------------------------------------------------------------------------------------------------------
def test_fast_build_under_reuse(monkeypatch):
    from pdp import native
    inst, runs = xr.mixed()
    batch, status, models, regions, plen, want = check_cases(0)
    switch(monkeypatch, 1)
    prev = native.use_build('fast')
    try:
        got = search(problem(inst), inst, 1, arena=12)
        verdicts = checked(problem(batch), 1, batch, status, models, regions, plen)
    finally:
        native.use_build(prev)
    same(got, runs[12])
    same_check(verdicts, want)
