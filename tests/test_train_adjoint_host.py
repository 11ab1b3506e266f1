"""What makes tests/test_train_adjoint_gpu.py mean something, checked without a GPU: the models of tests/train_adjoint_model.py equal the
CPU oracle's forward in fp32, their float64 autograd equals central differences of their float64 forward, and the inputs do what they
are for -- finite in both precisions, the same clamp decisions in both, every reachable clamp branch taken and not taken, gradients that
are mostly non-zero in every instance, and block-stride loops that take a second stride."""
import numpy as np
import pytest
import torch

import families
import train_adjoint_model as M

SP = [pytest.param(nm, case, id='%s-%s' % (nm, case)) for nm in M.BATCHES for case in M.SP_CASES]
LOSS = [pytest.param(nm, case, id='%s-%s' % (nm, case)) for nm in M.BATCHES for case in M.LOSS_CASES]
LOSS_F64 = [pytest.param(nm, case, id='%s-%s' % (nm, case)) for nm in M.BATCHES for case in M.LOSS_CASES_F64]
FD_H, FD_N, FD_BOUND = 1e-6, 200, 1e-6


def _problem(oracle, name):
    b = M.batch(name)
    return oracle.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])


# ---- model against oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,case', SP)
def test_sweep_model_in_fp32_equals_the_oracle(oracle, name, case):
    """q and eta of the fp32 model against orc_sp_propagate_adapted, the formulation the golden fixtures pin; the difference counted
    against the float64 model's largest magnitude.  Measured over all 80 cases: q at most 2.0e-7 (hub, pi 0.9), eta at most 6.2e-8 -- two
    or three ulp of the values near 1 (libm's expf / logf against torch's vectorised ones; the sums run in the same ascending edge order on
    both sides).  Bound: 4e-7."""
    b, ref = M.batch(name), M.sp_reference(name, case)
    inp, op = ref['inp'], _problem(oracle, name)
    em = inp['edge_mask']
    fs2 = torch.stack((inp['eta_in'], inp['force']), 1).numpy()
    oq, ofs = op.sp_propagate_adapted(inp['xlog'].numpy(), fs2, None if em is None else em.numpy(), np.ones(op.B, np.uint8),
                                      np.zeros((op.E, 3), np.float32), np.zeros((op.E, 2), np.float32), inp['pi'])
    q32, eta32 = ref['f32'][0], ref['f32'][1]
    dq = float((torch.from_numpy(oq).double() - q32.double()).abs().max() / ref['f64'][0].abs().max())
    de = float((torch.from_numpy(ofs[:, 0]).double() - eta32.double()).abs().max() / ref['f64'][1].abs().max())
    print('%s %s: q %.2e eta %.2e' % (name, case, dq, de))
    assert np.array_equal(ofs[:, 1], inp['force'].numpy())
    assert dq <= 4e-7 and de <= 4e-7, (dq, de)


@pytest.mark.parametrize('name,case', LOSS)
def test_loss_model_in_fp32_equals_the_oracle(oracle, name, case):
    """the fp32 model's loss against orc_sat_loss, counted against the float64 loss.  Measured: at most 3.7e-6 (long-257, 7 701 clauses: the
    oracle adds its clause terms one after the other in fp32, torch.mean adds them pairwise, and the float64 value lies within 1e-7 of the
    pairwise one).  Bound: 1e-5.  Where the fp32 loss is inf (eps 1e-8, sharpness 5) the oracle's is inf too."""
    ref, op = M.loss_reference(name, case), _problem(oracle, name)
    coeff, eps, sharp = M.LOSS_CASES[case]
    got, want, exact = op.sat_loss(ref['pred'].numpy(), coeff, eps, sharp), float(ref['f32'][0]), float(ref['f64'][0])
    if np.isinf(want):
        assert np.isinf(got) and got > 0
    else:
        print('%s %s: %.2e' % (name, case, abs(got - want) / abs(exact)))
        assert abs(got - want) <= 1e-5 * abs(exact), (got, want, exact)


# ---- model against itself -----------------------------------------------------------------------------------------------------------------
def _check_fd(pick, fd, inst, grad, B):
    "each sampled entry within FD_BOUND of its instance's largest gradient magnitude (O(h^2) truncation plus 1e-16 / h rounding)"
    scale = M.instance_max(grad.abs(), inst, B)[inst[pick]]
    return float(((grad[pick] - fd).abs() / scale).max())


@pytest.mark.parametrize('name,case', SP)
def test_sweep_model_autograd_equals_central_differences(name, case):
    """float64 autograd of the model against central differences (h = 1e-6) of its float64 forward in 200 random inputs -- 100 of xlog, 100 of
    eta_in with 1 - eta_in > 0.05, away from the log's clamp; no clause sum lies within 1 of 30.  The differences are taken per output
    element before the product with the upstream gradient, so the rounding is that of the elements an input reaches, not of a sum over
    the batch.  Measured: at most 1.2e-9 of the instance's largest gradient (the loss below: 3.3e-8)."""
    b, ref = M.batch(name), M.sp_reference(name, case)
    inp = ref['inp']
    gq, ge = inp['g_q'].double(), inp['g_eta'].double()
    rng = np.random.RandomState(7)
    assert not bool(((ref['t64']['agg'] - 30).abs() < 1).any())

    def forward(xlog, eta_in):
        with torch.no_grad():
            return M.sp_adapted(xlog, eta_in, inp['force'], inp['edge_mask'], b['gm'], b['sign'], b['V'], b['F'], inp['pi'], torch.float64)

    x0, e0 = inp['xlog'].double(), inp['eta_in'].double()
    worst = 0.0
    for which, base, grad, ok in ((0, x0, ref['f64'][2], torch.ones(b['E'], dtype=torch.bool)), (1, e0, ref['f64'][3], (1 - e0) > 0.05)):
        cand = ok.nonzero().flatten().numpy()
        pick = torch.from_numpy(rng.choice(cand, size=min(FD_N // 2, cand.size), replace=False))
        fd = torch.zeros(pick.numel(), dtype=torch.float64)
        for j, e in enumerate(pick.tolist()):
            outs = []
            for sgn in (1.0, -1.0):
                p = base.clone(); p[e] += sgn * FD_H
                outs.append(forward(p, e0) if which == 0 else forward(x0, p))
            fd[j] = (((outs[0][0] - outs[1][0]) * gq).sum() + ((outs[0][1] - outs[1][1]) * ge).sum()) / (2 * FD_H)
        worst = max(worst, _check_fd(pick, fd, b['edge_inst'], grad, ref['B']))
    print('%s %s: %.2e' % (name, case, worst))
    assert worst <= FD_BOUND, worst


@pytest.mark.parametrize('name,case', LOSS_F64)
def test_loss_model_autograd_equals_central_differences(name, case):
    "the same for the loss in 200 random variables with 0 < pred < 1 (a clause at its nom <= eps clamp holds none of them: all of its variables are 0 or 1)"
    b, ref = M.batch(name), M.loss_reference(name, case)
    coeff, eps, sharp = M.LOSS_CASES[case]
    p0, grad = ref['pred'].double(), ref['f64'][1]
    clamped_edges = ref['t64']['nom_clamped'][b['gm'][1]]
    inside = (p0 > 0) & (p0 < 1)
    assert not bool(inside[b['gm'][0][clamped_edges]].any())
    cand = inside.nonzero().flatten().numpy()
    pick = torch.from_numpy(np.random.RandomState(8).choice(cand, size=min(FD_N, cand.size), replace=False))
    fd = torch.zeros(pick.numel(), dtype=torch.float64)
    for j, v in enumerate(pick.tolist()):
        terms = []
        for sgn in (1.0, -1.0):
            p = p0.clone(); p[v] += sgn * FD_H
            tr = {}
            with torch.no_grad():
                M.sat_loss(p, b['gm'], b['sign'], b['F'], coeff, eps, sharp, torch.float64, tr)
            terms.append(tr['terms'])
        fd[j] = (terms[0] - terms[1]).sum() / b['F'] / (2 * FD_H)
    worst = _check_fd(pick, fd, b['var_inst'], grad, ref['B'])
    print('%s %s: %.2e' % (name, case, worst))
    assert worst <= FD_BOUND, worst


# ---- conditions on every case -------------------------------------------------------------------------------------------------------------
def _per_instance_any(x, inst, B):
    return M.instance_max((x != 0).double().reshape(x.shape[0], -1).amax(1), inst, B) > 0


@pytest.mark.parametrize('name,case', SP)
def test_sweep_inputs_are_finite_decided_alike_and_not_vacuous(name, case):
    b, ref = M.batch(name), M.sp_reference(name, case)
    kind, with_mask, pi = M.SP_CASES[case]
    for r in (ref['f32'], ref['f64']):
        for x in r:
            assert bool(torch.isfinite(x).all())
    # every clamp decision falls the same way in fp32 and float64
    for key in ('om_clamped', 'agg_clamped', 'same_clamped', 'opp_clamped', 'dc_clamped'):
        assert torch.equal(ref['t32'][key], ref['t64'][key]), key
    t = ref['t64']
    # same, opp and same + opp are sums of log(min(.., 1)) <= 0: their `< 30` branches cannot be false, whatever the input
    assert not bool(t['same_clamped'].any() or t['opp_clamped'].any() or t['dc_clamped'].any())
    if kind == 'clamp':
        for key in ('om_clamped', 'agg_clamped'):
            taken = int(t[key].sum())
            assert taken >= 5 and taken <= b['E'] // 2, (key, taken, b['E'])
        assert int((ref['inp']['eta_in'] == M.ETA_BELOW_ONE).sum()) >= (2 if name == 'minimal' else 5)
        assert int((ref['inp']['eta_in'] == 0).sum()) >= 4
        special = (ref['inp']['eta_in'] >= M.ETA_BELOW_ONE)
        assert int(torch.zeros(b['V']).index_add(0, b['gm'][0], special.float()).max()) == 1         # one edge at or just below 1 per variable
    else:
        assert not bool(t['om_clamped'].any() or t['agg_clamped'].any())
    if with_mask:
        em = ref['inp']['edge_mask']
        assert 0.15 < float((em == 0).float().mean()) < 0.3
        assert int(torch.ones(b['F']).scatter_reduce(0, b['gm'][1], em, 'amax', include_self=False).eq(0).sum()) >= 1      # a whole clause
        assert int(torch.ones(b['V']).scatter_reduce(0, b['gm'][0], em, 'amax', include_self=False).eq(0).sum()) >= 1      # a whole variable
    # at least 70 % of every compared gradient is non-zero.  Structural zeros are left out of the count: the edge of a unit clause has
    # dxlog = 0 (x enters no OTHER edge of its clause) and the only edge of a variable has deta_in = 0 (`minimal` is made of such rows)
    dxlog, deta = ref['f64'][2], ref['f64'][3]
    can_x = torch.from_numpy(b['len'][b['graph_map'][1]] >= 2)
    can_e = torch.from_numpy(b['deg'][b['graph_map'][0]] >= 2)
    fx, fe = float((dxlog[can_x] != 0).double().mean()), float((deta[can_e] != 0).double().mean())
    print('%s %s: non-zero dxlog %.2f deta_in %.2f, err_ref %s' % (name, case, fx, fe, ref['err_ref']))
    # (long-only-100 in the clamp cases: a quarter of its 100-literal clauses hold an xlog past the clamp, which zeroes the rest of the clause)
    assert fx >= (0.5 if (name == 'long-only-100' and kind == 'clamp') else 0.7) and fe >= 0.7, (fx, fe)
    # every instance has a non-zero gradient (an instance of one edge has none to give)
    edges = np.bincount(b['edge_inst'].numpy(), minlength=ref['B'])
    some = _per_instance_any(dxlog, b['edge_inst'], ref['B']) | _per_instance_any(deta, b['edge_inst'], ref['B'])
    assert bool((some | torch.from_numpy(edges <= 1)).all())


@pytest.mark.parametrize('name,case', LOSS)
def test_loss_inputs_are_finite_decided_alike_and_not_vacuous(name, case):
    b, ref = M.batch(name), M.loss_reference(name, case)
    coeff, eps, sharp = M.LOSS_CASES[case]
    t32, t64 = ref['t32'], ref['t64']
    assert torch.equal(t32['nom_clamped'], t64['nom_clamped']) and torch.equal(t32['cv_clamped'], t64['cv_clamped'])
    # cv = 1 + d^k with d = den / max(nom, eps) - 1 >= 0 (every weight is >= 1 and ev <= 1, so den >= nom and den >= 1 > eps): cv >= 1, and the
    # `cv > eps` branch cannot be false for eps < 1
    assert not bool(t64['cv_clamped'].any())
    taken = int(t64['nom_clamped'].sum())
    # `minimal` holds one clause 40 times and another 12 times: a falsified copy falsifies them all, and its two 50-clause instances are
    # all-positive and all-negative, so there the branch is taken on more than half of the 158 clauses; both sides still get 50 or more
    # long-only-100: one falsified clause per instance -- two clauses of 100 literals on 300 variables share some 33 of them and would have
    # to agree on every one
    assert taken >= (4 if name == 'long-only-100' else 5) and b['F'] - taken >= (50 if name == 'minimal' else (b['F'] + 1) // 2), (taken, b['F'])
    pred = ref['pred']
    for value in (0.0, 1.0, 0.5):
        assert int((pred == value).sum()) >= 1
    assert bool(torch.isfinite(ref['f64'][0])) and bool(torch.isfinite(ref['f64'][1]).all())
    l32, g32 = ref['f32']
    if case in M.LOSS_CASES_F64 or sharp == 1:
        assert bool(torch.isfinite(l32)) and bool(torch.isfinite(g32).all())
    else:
        # eps 1e-8, sharpness 5: a falsified clause has d = den / eps - 1 >= 1e8 and d^5 = inf in fp32: the loss is inf, the gradient through
        # such a clause exactly 0 -- and NaN (0 * inf) on every variable of a falsified clause of 35 literals or more, where d^4 overflows too
        assert bool(torch.isinf(l32)) and float(l32) > 0 and not bool(torch.isinf(g32).any())
        overflow4 = t64['nom_clamped'] & (torch.from_numpy(b['len']).double() / float(np.float32(eps)) - 1 > float(np.finfo(np.float32).max) ** 0.25)
        want_nan = torch.zeros(b['V']).index_add(0, b['gm'][0], overflow4[b['gm'][1]].float()) > 0
        assert torch.equal(torch.isnan(g32), want_nan)
        if name == 'long-257':                                   # (the long clause of the instances that have it at position 0 and 63)
            assert int(want_nan.sum()) == 2 * 257
    nz = float((ref['f64'][1] != 0).double().mean())
    deg0 = b['deg'] == 0
    assert nz >= 0.7 and bool((ref['f64'][1][torch.from_numpy(deg0)] == 0).all())
    assert bool(_per_instance_any(ref['f64'][1], b['var_inst'], ref['B']).all())
    print('%s %s: clamp taken %d / %d, non-zero %.2f, err_ref %.2e' % (name, case, taken, b['F'], nz, ref['err_ref']))


def test_the_spare_variables_are_there():
    b = M.batch(M.SPARE)
    rows = families.table(b)
    first = int(np.argmax(b['batch_variable_map'] == 1))
    assert [r['n'] for r in rows] == [40, 53, 70]
    assert sorted(np.nonzero(b['deg'] == 0)[0] - first) == [M.SPARE_AT[0], M.SPARE_AT[1], 52]


# which block-stride loops of the two kernels (256 threads per instance) take a second stride in at least one instance of the batch
STRIDES = {'minimal': (False, False, False), 'chains-100': (False, False, True), 'hub-254-255-256-257': (True, False, True), 'hub-1000': (True, False, True),
           'long-257': (True, True, True), 'long-only-100': (False, True, True), 'regular-4-3-n1000': (True, True, True),
           'ladder-4.2-n100-180': (True, False, True), 'power-0.5': (True, True, True), M.SPARE: (True, False, True)}


@pytest.mark.parametrize('name', M.BATCHES)
def test_which_loops_take_a_second_stride(name):
    rows = families.table(M.batch(name))
    got = (max(r['m'] for r in rows) > 256, max(r['n'] for r in rows) > 256, max(r['e'] for r in rows) > 256)
    assert got == STRIDES[name], got
    if name == 'regular-4-3-n1000':
        assert any(r['m'] > 1280 and r['n'] > 768 and r['e'] > 3840 for r in rows)        # six, four and sixteen strides in one instance
