"""The two graph-shaped adjoints of the training path -- k_sp_adapted_backward and k_sat_loss_grad, one 256-thread workgroup per instance,
block-stride loops over its clauses, variables and edges -- against the float64 models of tests/train_adjoint_model.py on structured
families (up to 1 001 variables, 1 332 clauses and 4 001 edges per instance: every loop takes several strides) and on the values where a
hand-written branch stands for a torch.max / torch.min of the reference (eta_in = 1, xlog past the clamp, falsified clauses, masked
edges).  tests/test_train_adjoint_host.py checks on the CPU that the models and the inputs are what they claim to be.

The error of a gradient is taken per instance (train_adjoint_model.instance_error); a kernel may reach four times the error of the
reference formulation's own fp32 autograd on the same inputs, and never less than 4e-6 (train_adjoint_model.bound).  Every test prints
its figures before it asserts (DESIGN.md section 4.6 holds the table).

Further down: the launch shapes of the neighbouring adjoints that no other test reaches -- a second stride of the grid-stride loops, the
GRU adjoint's row groups and column blocks at hidden 100 / 300 / 512, a first layer without a bias."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_adjoint_model as M
from helpers import random_batch
from test_families_gpu import ordered_row_sum
from test_hip_ops import t, npy, make_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SP = [pytest.param(nm, case, id='%s-%s' % (nm, case)) for nm in M.BATCHES for case in M.SP_CASES]
LOSS_F64 = [pytest.param(nm, case, id='%s-%s' % (nm, case)) for nm in M.BATCHES for case in M.LOSS_CASES_F64]
LOSS_F32 = [pytest.param(nm, case, id='%s-%s' % (nm, case)) for nm in M.BATCHES for case in M.LOSS_CASES_F32]

_PAIR = {}


def pair(oracle, name):
    if name not in _PAIR:
        _PAIR[name] = make_pair(oracle, M.batch(name))
    return _PAIR[name]


def nan_like(x):
    return torch.full_like(x, float('nan'))


def sp_backward_abi(hp, inp, dev_inp=None):
    "pdp_train_sp_adapted_backward called directly, both outputs pre-filled with NaN"
    from pdp import native
    d = dev_inp or sp_to_device(inp)
    dxlog, deta = nan_like(d['xlog']), nan_like(d['xlog'])
    native.check(native.lib().pdp_train_sp_adapted_backward(hp._h, native.ptr(d['xlog'], torch.float32), native.ptr(d['fs2'], torch.float32),
                                                            native.ptr(d['edge_mask'], torch.float32), C.c_float(inp['pi']), native.ptr(d['g_q'], torch.float32),
                                                            native.ptr(d['g_eta'], torch.float32), native.ptr(dxlog), native.ptr(deta), native._stream()))
    return dxlog, deta


def sp_to_device(inp):
    d = {k: (None if inp[k] is None else inp[k].to(DEV).contiguous()) for k in ('xlog', 'edge_mask', 'g_q', 'g_eta')}
    d['fs2'] = torch.stack((inp['eta_in'], inp['force']), 1).to(DEV).contiguous()
    return d


def loss_grad_abi(hp, pred_dev, case):
    from pdp import native
    coeff, eps, sharp = M.LOSS_CASES[case]
    dpred = nan_like(pred_dev)
    native.check(native.lib().pdp_sat_loss_grad(hp._h, native.ptr(pred_dev, torch.float32), C.c_float(coeff), C.c_float(eps), C.c_int(sharp), C.c_float(1.0),
                                                native.ptr(dpred), native._stream()))
    return dpred


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,case', SP)
def test_sweep_adjoint_against_float64(oracle, name, case):
    """dxlog and deta_in of train_ops.SpAdaptedSweep against float64 autograd of the model, and the same from a direct call of the ABI
    function into NaN-filled buffers: every element comes back finite, and equal to what the autograd.Function returned.  `dy` is
    deta_in (1 - eta_in): see train_adjoint_model.sp_reference.  The forward's q and fs equal the oracle's bit for bit (they are not held
    to the float64 bound: on a hub of 1 000 edges the reference's own fp32 q is 2e-5 off, exp of a sum of 1 000 terms)."""
    from pdp.nn import train_ops as T
    hp, op = pair(oracle, name)
    ref = M.sp_reference(name, case)
    inp = ref['inp']
    d = sp_to_device(inp)
    xlog = d['xlog'].clone().requires_grad_(True)
    eta_in = inp['eta_in'].to(DEV).requires_grad_(True)
    q, fs = T.SpAdaptedSweep.apply(xlog, torch.stack((eta_in, d['fs2'][:, 1]), 1), hp, d['edge_mask'], inp['pi'])
    ((q * d['g_q']).sum() + (fs[:, 0] * d['g_eta']).sum()).backward()
    em = inp['edge_mask']
    oq, ofs = op.sp_propagate_adapted(inp['xlog'].numpy(), npy(d['fs2']), None if em is None else em.numpy(), np.ones(op.B, np.uint8),
                                      np.zeros((op.E, 3), np.float32), np.zeros((op.E, 2), np.float32), inp['pi'])
    np.testing.assert_array_equal(npy(q), oq)
    np.testing.assert_array_equal(npy(fs), ofs)
    dxlog, deta = sp_backward_abi(hp, inp, d)
    assert bool(torch.isfinite(dxlog).all()) and bool(torch.isfinite(deta).all())
    assert torch.equal(dxlog, xlog.grad) and torch.equal(deta, eta_in.grad)
    err = M.sp_errors(ref, name, dxlog.cpu(), deta.cpu())
    for key in ('dxlog', 'deta_in', 'dy'):
        print('FIG sweep %s %s %s kernel %.3e err_ref %.3e ratio %.2f bound %.3e' % (name, case, key, err[key], ref['err_ref'][key],
                                                                                   err[key] / max(ref['err_ref'][key], 1e-30), M.bound(ref['err_ref'][key])))
    for key in ('dxlog', 'deta_in', 'dy'):
        assert err[key] <= M.bound(ref['err_ref'][key]), (key, err[key], ref['err_ref'][key])
    if inp['edge_mask'] is not None:
        masked = (inp['edge_mask'] == 0)
        assert bool((dxlog.cpu()[masked] == 0).all()) and bool((deta.cpu()[masked] == 0).all())
    assert bool((deta.cpu()[ref['t64']['om_clamped']] == 0).all())


# ---- the loss -------------------------------------------------------------------------------------------------------------------------------
def _loss_both_ways(hp, ref, case):
    "dpred through train_ops.SatLoss and through the ABI into a NaN-filled buffer: the same bits; returns (loss, dpred) on the CPU"
    from pdp.nn import train_ops as T
    coeff, eps, sharp = M.LOSS_CASES[case]
    x = ref['pred'].to(DEV).requires_grad_(True)
    loss = T.SatLoss.apply(x, hp, coeff, eps, sharp)
    loss.backward()
    dpred = loss_grad_abi(hp, x.detach(), case)
    assert torch.equal(torch.nan_to_num(dpred, nan=7.0), torch.nan_to_num(x.grad, nan=7.0))
    return loss.detach().cpu(), dpred.cpu()


@pytest.mark.parametrize('name,case', LOSS_F64)
def test_loss_adjoint_against_float64(oracle, name, case):
    "dpred of train_ops.SatLoss / pdp_sat_loss_grad against float64 autograd of the model; every element written, exactly 0 on a variable without edges"
    hp, op = pair(oracle, name)
    b, ref = M.batch(name), M.loss_reference(name, case)
    loss, dpred = _loss_both_ways(hp, ref, case)
    assert bool(torch.isfinite(dpred).all())
    assert bool((dpred[torch.from_numpy(b['deg'] == 0)] == 0).all())
    assert abs(float(loss) - float(ref['f64'][0])) <= 1e-5 * abs(float(ref['f64'][0]))
    err = M.instance_error(dpred, ref['f64'][1], b['var_inst'], ref['B'])
    print('FIG loss %s %s dpred kernel %.3e err_ref %.3e ratio %.2f bound %.3e' % (name, case, err, ref['err_ref'], err / max(ref['err_ref'], 1e-30), M.bound(ref['err_ref'])))
    assert err <= M.bound(ref['err_ref']), (err, ref['err_ref'])


@pytest.mark.parametrize('name,case', LOSS_F32)
def test_loss_adjoint_keeps_fp32_semantics_at_the_trainers_eps(oracle, name, case):
    """eps = 1e-8 (the trainer's): a falsified clause has d = den / eps - 1 >= 1e8, and with sharpness 5 fp32 overflows -- loss inf, the
    gradient through the clause exactly 0, NaN where d^4 overflows as well (a falsified clause of 35 literals or more) -- while float64
    gives a finite gradient of order 1 there.  The reference trains in fp32, so the fp32 model is the yardstick: the same NaN pattern, inf
    where its loss is inf, and the finite entries within max(4 e, 4e-6) of it, e = the fp32 model's own error against float64 on the
    clauses that do not overflow."""
    hp, op = pair(oracle, name)
    b, ref = M.batch(name), M.loss_reference(name, case)
    loss, dpred = _loss_both_ways(hp, ref, case)
    l32, g32 = ref['f32']
    assert not bool(torch.isinf(dpred).any())
    assert torch.equal(torch.isnan(dpred), torch.isnan(g32))
    assert bool((dpred[torch.from_numpy(b['deg'] == 0)] == 0).all())
    if bool(torch.isinf(l32)):
        assert bool(torch.isinf(loss)) and float(loss) > 0
    else:
        assert abs(float(loss) - float(l32)) <= 1e-5 * abs(float(l32))
    fin = torch.isfinite(g32)
    zero = torch.zeros_like(g32)
    err = M.instance_error(torch.where(fin, dpred, zero), torch.where(fin, g32, zero), b['var_inst'], ref['B'])
    print('FIG loss32 %s %s dpred kernel-vs-fp32 %.3e e %.3e ratio %.2f bound %.3e nan %d' % (name, case, err, ref['err_ref'], err / max(ref['err_ref'], 1e-30),
                                                                                            M.bound(ref['err_ref']), int((~fin).sum())))
    assert err <= M.bound(ref['err_ref']), (err, ref['err_ref'])


# ---- the two adjoints share ws_f and ws_v ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['minimal', 'hub-1000', 'regular-4-3-n1000', M.SPARE])
def test_the_two_adjoints_back_to_back_on_one_handle(oracle, name):
    "sweep adjoint then loss gradient on the same problem handle and stream, then the other order: the bits of each one called alone"
    b = M.batch(name)
    inp, lref = M.sp_reference(name, 'clamp-pi0.1')['inp'], M.loss_reference(name, 'k2-eps1e-3-s5')
    d, pred = sp_to_device(inp), lref['pred'].to(DEV)
    alone_sp = sp_backward_abi(make_pair(oracle, b)[0], inp, d)
    alone_loss = loss_grad_abi(make_pair(oracle, b)[0], pred, 'k2-eps1e-3-s5')
    hp = make_pair(oracle, b)[0]
    for order in ('sp-loss', 'loss-sp', 'sp-loss'):
        if order == 'sp-loss':
            got_sp = sp_backward_abi(hp, inp, d); got_loss = loss_grad_abi(hp, pred, 'k2-eps1e-3-s5')
        else:
            got_loss = loss_grad_abi(hp, pred, 'k2-eps1e-3-s5'); got_sp = sp_backward_abi(hp, inp, d)
        assert torch.equal(got_sp[0], alone_sp[0]) and torch.equal(got_sp[1], alone_sp[1]), order
        assert torch.equal(got_loss, alone_loss), order
    assert bool(torch.isfinite(alone_loss).all()) and bool(torch.isfinite(alone_sp[0]).all())


# ---- RowAggregate's adjoint on the same families ------------------------------------------------------------------------------------------------
def _row_aggregate_case(hp, rows, nrows, x, g, by_variable, include_self):
    """forward and adjoint of train_ops.RowAggregate on the device, the host's ordered sums of both, and the two sides of
    <A x, g> = <x, A^T g> accumulated in float64 from the device's fp32 results"""
    from pdp.nn import train_ops as T
    xs = t(x).requires_grad_(True)
    out = T.RowAggregate.apply(xs, hp, by_variable, include_self)
    out.backward(t(g))
    if include_self:
        want_out, want_ds = ordered_row_sum(rows, nrows, x), g[rows]                       # A^T g: every edge gets its row's g
    else:
        want_out, want_ds = ordered_row_sum(rows, nrows, x)[rows] - x, ordered_row_sum(rows, nrows, g)[rows] - g
    np.testing.assert_array_equal(npy(out), want_out)
    np.testing.assert_array_equal(npy(xs.grad), want_ds)
    lhs = float((out.detach().double() * t(g).double()).sum()), float((out.detach().double() * t(g).double()).abs().sum())
    rhs = float((xs.detach().double() * xs.grad.double()).sum())
    return lhs[0], rhs, lhs[1]


@pytest.mark.parametrize('A', [50, 51])
@pytest.mark.parametrize('by_variable,include_self', [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize('name', M.BATCHES)
def test_row_aggregate_adjoint_on_the_families(oracle, name, by_variable, include_self, A):
    """the adjoint of the ordered row sums equals the ordered transpose sum of the host bit for bit (include_self: a gather; else the row sum
    of the gradient minus the edge's own), and <A x, g> = <x, A^T g> in float64 within max(4 x the same identity's defect for torch's fp32
    index_add, 4e-6) of sum |A x . g|"""
    hp, op = pair(oracle, name)
    b = M.batch(name)
    rows = b['graph_map'][0 if by_variable else 1].astype(np.int64)
    nrows = b['V'] if by_variable else b['F']
    rng = np.random.RandomState(A + 2 * by_variable + include_self)
    x = (rng.randn(b['E'], A) * 0.5).astype(np.float32)
    g = rng.randn(nrows if include_self else b['E'], A).astype(np.float32)
    lhs, rhs, scale = _row_aggregate_case(hp, rows, nrows, x, g, by_variable, include_self)
    # the same identity for torch's fp32 index_add on the CPU
    xr, gr, rt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(g), torch.from_numpy(rows)
    agg = torch.zeros(nrows, A).index_add(0, rt, xr)
    outr = agg if include_self else agg[rt] - xr
    outr.backward(gr)
    ref_defect = abs(float((outr.detach().double() * gr.double()).sum()) - float((xr.detach().double() * xr.grad.double()).sum())) / scale
    defect = abs(lhs - rhs) / scale
    print('FIG rowagg %s var=%d self=%d A=%d defect %.3e ref %.3e' % (name, by_variable, include_self, A, defect, ref_defect))
    assert defect <= M.bound(ref_defect), (defect, ref_defect)


# ---- C. launch shapes next to them -----------------------------------------------------------------------------------------------------------
def _rel_to_max(a, r):
    return float((a.detach().double().cpu() - r.detach().cpu()).abs().max() / r.detach().abs().max().clamp(min=1e-30))


def _leaf(*shape, scale=0.3, seed=0):
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).requires_grad_(True)


@pytest.mark.parametrize('by_variable,include_self,A', [(True, False, 16), (False, False, 16), (True, True, 16), (False, True, 42)])
def test_row_aggregate_past_one_pass_of_the_grid(oracle, by_variable, include_self, A):
    """grid1d caps a launch at 16 384 x 256 threads.  120 instances of uniform 3-SAT (n 200, m 840: 302 400 edges) at A = 16 are 4.8 M
    elements: k_trow_spread takes a second stride in the exclude-self forward and in both adjoints.  k_trow_sum has one thread per
    (row, column); its second stride needs 100 800 clause rows x 42 columns."""
    b = random_batch(batch=120, n=200, k=3, m=840, seed=300)
    hp, op = make_pair(oracle, b)
    assert hp.E * 16 > 16384 * 256 and (A == 16 or hp.F * A > 16384 * 256)
    rows = b['graph_map'][0 if by_variable else 1].astype(np.int64)
    nrows = hp.V if by_variable else hp.F
    rng = np.random.RandomState(A)
    x = (rng.randn(hp.E, A) * 0.5).astype(np.float32)
    g = rng.randn(nrows if include_self else hp.E, A).astype(np.float32)
    _row_aggregate_case(hp, rows, nrows, x, g, by_variable, include_self)


def _gru_against_float64(cell, got, x_parts, h, g):
    "float64 torch.nn.GRUCell on the same inputs: everything within 4e-6 of the tensor's largest magnitude"
    import copy
    cd = copy.deepcopy(cell).double().cpu()
    for p_ in cd.parameters():
        p_.grad = None
    parts = [p_.detach().double().cpu().requires_grad_(p_.requires_grad) for p_ in x_parts]
    hd = h.detach().double().cpu().requires_grad_(True)
    hr = cd(torch.cat(parts, 1) if len(parts) > 1 else parts[0], hd)
    hr.backward(g.double().cpu())
    ref = [hr.detach(), parts[0].grad, hd.grad] + [p_.grad for p_ in cd.parameters()]
    for a, r, name in zip(got, ref, ('h', 'dx', 'dh', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh')):
        e = _rel_to_max(a, r)
        print('FIG gru %s %.3e' % (name, e))
        assert e < 4e-6, (name, e)


@pytest.mark.parametrize('R,Kx,H', [(33000, 129, 128), (777, 101, 100), (777, 301, 300), (777, 513, 512)])
def test_gru_cell_adjoint_launch_shapes_against_float64(R, Kx, H):
    """train_ops.GruCell without packed weights (two GEMMs, k_gru_point, k_gru_point_backward): 33 000 x 128 is past one pass of k_gru_point's
    grid; hidden 100 gives the adjoint two row groups and 56 idle lanes, 300 two column blocks (the second one ragged), 512 two full ones"""
    from pdp.nn import train_ops as T
    torch.manual_seed(H)
    cell = torch.nn.GRUCell(Kx, H).to(DEV)
    x, h = _leaf(R, Kx, seed=4), _leaf(R, H, seed=5)
    g = torch.randn(R, H, device=DEV)
    hn = T.GruCell.apply(x, h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)
    hn.backward(g)
    _gru_against_float64(cell, [hn, x.grad, h.grad] + [p_.grad for p_ in cell.parameters()], [x], h, g)


@pytest.mark.parametrize('H', [100, 300, 512])
def test_gru_adjoint_with_the_sign_column_apart_at_other_widths(H):
    """pdp_train_gru_backward_s (input = [state [R, H] | sign [R]] held apart; train_ops.GruCellS is wired to hidden 128) called directly at
    hidden 100 / 300 / 512, R = 777, on the gates saved by pdp_train_gru: against float64 GRUCell on the concatenation"""
    from pdp import native
    R, Ks = 777, H
    torch.manual_seed(H + 1)
    cell = torch.nn.GRUCell(Ks + 1, H).to(DEV)
    state, h = _leaf(R, Ks, seed=21), _leaf(R, H, seed=22)
    sign = torch.sign(torch.randn(R, device=DEV))
    g = torch.randn(R, H, device=DEV)
    L, P = native.lib(), native.ptr
    w_ih, w_hh, b_ih, b_hh = [p_.detach().contiguous() for p_ in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)]
    x = torch.cat((state.detach(), sign.unsqueeze(1)), 1).contiguous()
    hd = h.detach().contiguous()
    new = lambda *sh: torch.full(sh, float('nan'), dtype=torch.float32, device=DEV)      # noqa: E731
    hn, saved, scratch = new(R, H), new(R, 4 * H), new(R, 6 * H)
    native.check(L.pdp_train_gru(P(x, torch.float32), P(hd, torch.float32), P(w_ih), P(w_hh), P(b_ih), P(b_hh), C.c_int64(R), C.c_int(Ks + 1), C.c_int(H), P(hn),
                                 P(saved), P(scratch), native._stream()))
    dstate, dh, dw_ih, dw_hh, db_ih, db_hh = new(R, Ks), new(R, H), new(3 * H, Ks + 1), new(3 * H, H), new(3 * H), new(3 * H)
    scratch = new(R, 6 * H)
    native.check(L.pdp_train_gru_backward_s(P(g, torch.float32), P(saved), P(state.detach().contiguous()), P(sign.contiguous()), P(hd), P(w_ih), P(w_hh),
                                            C.c_int64(R), C.c_int(Ks), C.c_int(H), P(dstate), P(dh), P(dw_ih), P(dw_hh), P(db_ih), P(db_hh), P(scratch),
                                            native._stream()))
    for out in (hn, dstate, dh, dw_ih, dw_hh, db_ih, db_hh):
        assert bool(torch.isfinite(out).all())
    _gru_against_float64(cell, [hn, dstate, dh, dw_ih, dw_hh, db_ih, db_hh], [state, sign.unsqueeze(1)], h, g)


@pytest.mark.parametrize('R,K,N,act,x_grad', [(50000, 51, 100, 'logsigmoid', True), (50000, 51, 100, 'logsigmoid', False), (1000, 33, 100, 'relu', False),
                                               (4100, 129, 50, 'none', False)])
def test_linear_without_a_bias_against_float64(R, K, N, act, x_grad):
    """train_ops.LinearAct with bias=None: dZ comes from k_act_backward (no column-sum pass) -- 50 000 x 100 is past one pass of its grid --,
    and on an input that needs no gradient (a first layer) the adjoint gets dX = NULL.  Against float64 F.linear, 4e-6 of the largest
    magnitude."""
    from pdp.nn import train_ops as T
    fn = {'logsigmoid': F.logsigmoid, 'relu': torch.relu, 'none': lambda z: z}[act]
    x, w = _leaf(R, K, seed=1), _leaf(N, K, seed=2)
    if not x_grad:
        x = x.detach()
    g = torch.randn(R, N, device=DEV)
    y = T.LinearAct.apply(x, w, None, act)
    y.backward(g)
    assert x_grad or x.grad is None
    xd, wd = x.detach().double().cpu().requires_grad_(x_grad), w.detach().double().cpu().requires_grad_(True)
    yr = fn(F.linear(xd, wd))
    yr.backward(g.double().cpu())
    pairs = [(y, yr, 'y'), (w.grad, wd.grad, 'dw')] + ([(x.grad, xd.grad, 'dx')] if x_grad else [])
    for a, r, name in pairs:
        e = _rel_to_max(a, r)
        print('FIG linear %s %.3e' % (name, e))
        assert e < 4e-6, (name, e)
