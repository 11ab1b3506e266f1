"""Plain-torch CPU models of the two graph-shaped adjoints of the training path, and the inputs they are compared on (a plain module like
exact_model.py; tests/test_train_adjoint_host.py checks the models and the inputs, tests/test_train_adjoint_gpu.py the kernels).

``sp_adapted`` is the adaptor form of the SP sweep (reference: pdp_propagate.py:163-221, no active mask) and ``sat_loss`` the energy loss
(reference: util.py:178-197), both written with index_add for the sparse products and with torch.max / torch.min where the reference has
them, so that autograd gives the gradient to the winning side exactly as it does there.  Both take a dtype: float64 is the yardstick of
the kernels' adjoints, float32 is "what the reference computes" (its own rounding error, and its semantics where fp32 overflows).

The leaves are the kernels' own inputs -- xlog, eta_in, pred -- promoted exactly from fp32, never the pre-activations behind them: fp32
sigmoid(40) is exactly 1 and the sweep clamps log(1 - eta) there, float64 sigmoid(40) is 1 - 4e-18 and does not, and a model started
from the pre-activation would be a different function.  For the same reason the constants (1e-40, 30, pi, coeff, eps) are rounded to fp32
first and promoted.
"""
import numpy as np
import torch
import torch.nn.functional as F

import families
import helpers  # noqa: F401  (sys.path)
from pdp import generator
from pdp.factorgraph import dataset

SP_EPS, SP_MAX = 1e-40, 30.0


def _c(value, dtype):
    "a constant the way the fp32 code sees it, in the model's dtype"
    return torch.tensor(float(np.float32(value)), dtype=torch.float32).to(dtype)


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def sp_adapted(xlog, eta_in, force, edge_mask, graph_map, sign, V, F_, pi, dtype, trace=None):
    """xlog, eta_in [E] of ``dtype`` (the leaves); force, sign [E] (+-1), edge_mask [E] or None, graph_map [2,E] int64.
    Returns (q [E,3], eta [E]).  ``trace``: a dict that receives every clamp decision of the sweep as a bool tensor."""
    assert xlog.dtype == dtype and eta_in.dtype == dtype
    eps, mx = _c(SP_EPS, dtype), _c(SP_MAX, dtype)
    s, force = sign.to(dtype), force.to(dtype)
    em = None if edge_mask is None else edge_mask.to(dtype)
    var, fn = graph_map[0], graph_map[1]
    safe_log = lambda a: torch.max(a, eps).log()      # noqa: E731
    safe_exp = lambda a: torch.min(a, mx).exp()       # noqa: E731
    x = xlog if em is None else xlog * em
    S = torch.zeros(F_, dtype=dtype).index_add(0, fn, x)
    agg = S[fn] - x
    eta = safe_exp(agg)
    om = 1 - eta_in
    y = safe_log(om)
    if em is not None:
        y = y * em
    P = torch.zeros(V, dtype=dtype).index_add(0, var, y * (s > 0).to(dtype))[var]
    N = torch.zeros(V, dtype=dtype).index_add(0, var, y * (s < 0).to(dtype))[var]
    lg = lambda c: safe_log(1.0 - _c(pi, dtype) * c.to(dtype))      # noqa: E731
    same = 0.5 * (1 + s) * P + 0.5 * (1 - s) * N - y + lg(force == s)
    opp = 0.5 * (1 - s) * P + 0.5 * (1 + s) * N + lg(force == -s)
    dc = safe_exp(same + opp)
    A, B = safe_exp(same), safe_exp(opp)
    qu, qs = A * (1 - B), B * (1 - A)
    tot = qu + qs + dc
    if trace is not None:
        trace.update(om_clamped=(om <= eps).detach(), agg_clamped=(agg >= mx).detach(), same_clamped=(same >= mx).detach(),
                     opp_clamped=(opp >= mx).detach(), dc_clamped=(same + opp >= mx).detach(), tot=tot.detach(), agg=agg.detach())
    return torch.stack((qu, qs, dc), 1) / tot.unsqueeze(1), eta


def sat_loss(pred, graph_map, sign, F_, coeff, eps, sharpness, dtype, trace=None):
    "pred [V] of ``dtype`` (the leaf).  Returns the scalar loss; ``trace`` receives the per-clause terms and the two clamp decisions."""
    assert pred.dtype == dtype
    s = sign.to(dtype)
    e_, k_ = _c(eps, dtype), _c(coeff, dtype)
    ev = s * pred[graph_map[0]] + (1 - s) / 2
    w = (k_ * ev).exp()
    nom = torch.zeros(F_, dtype=dtype).index_add(0, graph_map[1], w * ev)
    den = torch.zeros(F_, dtype=dtype).index_add(0, graph_map[1], w)
    cv = 1 + (den / torch.max(nom, e_) - 1).pow(int(sharpness))
    terms = torch.max(cv, e_).log()
    if trace is not None:
        trace.update(nom_clamped=(nom <= e_).detach(), cv_clamped=(cv <= e_).detach(), terms=terms.detach(), cv=cv.detach())
    return terms.mean()


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
FAMILIES = ['minimal', 'chains-100', 'hub-254-255-256-257', 'hub-1000', 'long-257', 'long-only-100', 'regular-4-3-n1000', 'ladder-4.2-n100-180',
            'power-0.5']
SPARE = 'spare-variables'
BATCHES = FAMILIES + [SPARE]
SPARE_AT = (7, 30)           # 0-based variable ids of instance 1 that no clause uses; a third one is the instance's last variable


def _spare_batch():
    """three uniform 3-SAT instances (n = 40, 50, 70; m = 168, 210, 294); the second one is declared with three more variables than its
    clauses use -- two inside the id range, one at its end"""
    items = []
    for i, n in enumerate((40, 50, 70)):
        vn, fn, gm, ef, lab, nm = dataset.instance_from_clauses(n, generator.uniform_ksat(n, int(round(4.2 * n)), 3, np.random.RandomState(14000 + i)),
                                                                label=-1, name='spare%d' % i)
        if i == 1:
            gm = gm.copy()
            for at in SPARE_AT:
                gm[0, gm[0] >= at] += 1
            vn += 3
        items.append((vn, fn, gm, ef, lab, nm))
    return dataset.collate_segment(items)


_CACHE = {}


def batch(name):
    "the collated numpy batch plus what the builders and the error measure need, cached"
    if name not in _CACHE:
        b = dict(_spare_batch() if name == SPARE else families.batch(name))
        gm = b['graph_map'].astype(np.int64)
        b['E'], b['V'], b['F'] = gm.shape[1], b['batch_variable_map'].size, b['batch_function_map'].size
        b['deg'] = np.bincount(gm[0], minlength=b['V'])
        b['len'] = np.bincount(gm[1], minlength=b['F'])
        b['gm'] = torch.from_numpy(gm)
        b['sign'] = torch.from_numpy(b['edge_feature'].reshape(-1).astype(np.float32))
        b['var_inst'] = torch.from_numpy(b['batch_variable_map'].astype(np.int64))
        b['edge_inst'] = b['var_inst'][b['gm'][0]]
        # first edge (lowest edge id) of every variable, -1 for a variable without edges
        first = np.full(b['V'], -1, np.int64)
        first[gm[0][::-1]] = np.arange(b['E'])[::-1]
        b['first_edge'] = first
        _CACHE[name] = b
    return _CACHE[name]


def _seed(name, salt):
    import zlib
    return (zlib.crc32(name.encode()) ^ (salt * 0x9e3779b1)) & 0x7fffffff


# ---- inputs of the sweep -----------------------------------------------------------------------------------------------------------------
# case id -> (kind of values, with the edge mask, pi); pi = 1 is left out: q is one-hot there and the true deta_in (1e-12) is below the
# reference's own cancellation noise
SP_CASES = {'interior-pi0': ('interior', False, 0.0), 'interior-pi0.1': ('interior', False, 0.1), 'interior-pi0.9': ('interior', False, 0.9),
            'interior-mask-pi0.1': ('interior', True, 0.1),
            'clamp-pi0': ('clamp', True, 0.0), 'clamp-pi0.1': ('clamp', True, 0.1), 'clamp-pi0.9': ('clamp', True, 0.9),
            'clamp-nomask-pi0.1': ('clamp', False, 0.1)}
ETA_BELOW_ONE = float(np.float32(1) - np.float32(2.0 ** -24))       # the largest fp32 below 1
SAT_RESIDUE, ZERO_RESIDUE = 8, 3                                   # eta_in = 1 / 0 on the first edge of the variables 8 / 3 mod 10
XLOG_PAST = 35.0                                                   # past the exp(min(., 30)) clamp of the clause sums


def sp_inputs(name, case):
    """dict of fp32 CPU tensors: xlog, eta_in, force [E], edge_mask [E] or None, g_q [E,3], g_eta [E], and pi.

    interior: xlog = logsigmoid(z), z = N(0,1) + log(len(clause(e))) + 1;  eta_in = sigmoid(u), u = N(0,1) - log(deg(var(e))) - 1: the
    scaling keeps a hub's sum of 1 000 logs inside fp32's range (unscaled N(0,2) draws give tot = 0 and NaN in the reference's own fp32
    forward on hub-1000).
    clamp: on top of it eta_in = 1 on the first edge of every 10th variable (8 mod 10), 0 on the first edge of the variables 3 mod 10, the largest
    fp32 below 1 on a further 1 % of the edges (the divisor of the gradient is 6e-8 there), xlog = 35 on 2 % of the edges.  A variable
    holds at most one edge at or just below 1: with two of them tot falls to 1e-15 ... 1e-40 and the reference's own fp32 autograd is
    noise or NaN (measured: 24.6 for a true 2e-8 on a hub with one edge at 1 and three just below).
    mask: 20 % zeros, plus one whole clause and one whole variable."""
    kind, with_mask, pi = SP_CASES[case]
    b = batch(name)
    E, gm = b['E'], b['graph_map'].astype(np.int64)
    rng = np.random.RandomState(_seed(name, 1))                   # the same draws for every case of a family
    z = rng.randn(E) + np.log(b['len'][gm[1]]) + 1.0
    u = rng.randn(E) - np.log(b['deg'][gm[0]]) - 1.0
    force = np.where(rng.rand(E) < 0.5, -1.0, 1.0)
    g_q, g_eta = rng.randn(E, 3), rng.randn(E)
    mask = (rng.rand(E) >= 0.2).astype(np.float32)
    # one whole clause and one whole variable, the first ones of the last instance with two edges or more
    last_f, last_v = b['batch_function_map'] == b['batch_function_map'].max(), b['batch_variable_map'] == b['batch_variable_map'].max()
    mask[gm[1] == int(np.argmax(last_f & (b['len'] >= 2)))] = 0
    mask[gm[0] == int(np.argmax(last_v & (b['deg'] >= 2)))] = 0
    pick_below = rng.rand(E) < 0.01
    # 2 to 3 % of the edges, all of them in every 4th clause: every other edge of such a clause takes the clamp, and with 100 literals per
    # clause an even spread would leave no clause without one
    pick_past = (rng.rand(E) < 0.04) & (gm[1] % 4 == 0)
    first_of_clause = np.full(b['F'], -1, np.int64)
    first_of_clause[gm[1][::-1]] = np.arange(E)[::-1]
    pick_past[first_of_clause[(np.arange(b['F']) % 16 == 0) & (b['len'] >= 2)]] = True      # and the first edge of every 16th clause
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    xlog, eta_in = F.logsigmoid(f32(z)), torch.sigmoid(f32(u))
    if kind == 'clamp':
        first, v = b['first_edge'], np.arange(b['V'])
        one = first[(v % 10 == SAT_RESIDUE) & (first >= 0)]
        zero = first[(v % 10 == ZERO_RESIDUE) & (first >= 0)]
        eta_in[torch.from_numpy(one)] = 1.0
        eta_in[torch.from_numpy(zero)] = 0.0
        # the edges just below 1: none on a variable that holds a saturated edge, and one per variable (a hub would collect ten of them)
        pick_below[zero] = False
        pick_below[v[gm[0]] % 10 == SAT_RESIDUE] = False
        below = np.nonzero(pick_below)[0]
        below = below[np.unique(gm[0][below], return_index=True)[1]]
        eta_in[torch.from_numpy(below)] = ETA_BELOW_ONE
        xlog[torch.from_numpy(np.nonzero(pick_past)[0])] = XLOG_PAST
    return dict(xlog=xlog, eta_in=eta_in, force=f32(force), edge_mask=f32(mask) if with_mask else None, g_q=f32(g_q), g_eta=f32(g_eta), pi=pi)


def sp_run(name, inp, dtype, trace=None):
    "forward and autograd of the model in ``dtype``: (q, eta, dxlog, deta_in), detached"
    b = batch(name)
    xlog = inp['xlog'].detach().to(dtype).clone().requires_grad_(True)
    eta_in = inp['eta_in'].detach().to(dtype).clone().requires_grad_(True)
    q, eta = sp_adapted(xlog, eta_in, inp['force'], inp['edge_mask'], b['gm'], b['sign'], b['V'], b['F'], inp['pi'], dtype, trace)
    ((q * inp['g_q'].to(dtype)).sum() + (eta * inp['g_eta'].to(dtype)).sum()).backward()
    return q.detach(), eta.detach(), xlog.grad, eta_in.grad


# ---- inputs of the loss ------------------------------------------------------------------------------------------------------------------
# (coeff, eps, sharpness): against float64 ...
LOSS_CASES_F64 = {'k2-eps1e-3-s5': (2.0, 1e-3, 5), 'k10-eps1e-3-s2': (10.0, 1e-3, 2), 'k1-eps1e-3-s1': (1.0, 1e-3, 1)}
# ... and the trainer's own eps, where a falsified clause overflows fp32 (d = den / eps - 1 = 3e8, d^5 = inf) and the reference's fp32
# arithmetic, not float64, is what training computes
LOSS_CASES_F32 = {'k10-eps1e-8-s5': (10.0, 1e-8, 5), 'k2-eps1e-8-s1': (2.0, 1e-8, 1)}
LOSS_CASES = dict(LOSS_CASES_F64, **LOSS_CASES_F32)


def loss_inputs(name):
    """pred [V] fp32: uniform in (0.05, 0.95); 15 % exactly 1, 15 % exactly 0, 5 % exactly 0.5; then every 7th clause is falsified exactly (0
    under its positive literals, 1 under its negative ones: ev = 0 and nom = 0 exactly in any precision).  A clause whose variables an
    earlier falsified clause has set the other way is left alone (it would undo that one), and so is every clause that would take the
    falsified clauses past half of its instance's variables (the first one of an instance is always taken): a hub instance has 19 clauses
    per variable, and without the limit no variable of it would keep an interior value."""
    b = batch(name)
    gm, sgn = b['graph_map'].astype(np.int64), b['edge_feature'].reshape(-1)
    rng = np.random.RandomState(_seed(name, 2))
    pred = rng.uniform(0.05, 0.95, size=b['V'])
    r = rng.rand(b['V'])
    pred[r < 0.15] = 1.0
    pred[(r >= 0.15) & (r < 0.30)] = 0.0
    pred[(r >= 0.30) & (r < 0.35)] = 0.5
    order = np.argsort(gm[1], kind='stable')
    ptr = np.r_[0, np.cumsum(b['len'])]
    fixed = np.zeros(b['V'], bool)
    n_inst = np.bincount(b['batch_variable_map'])
    used = np.zeros(n_inst.size, np.int64)
    for c in range(0, b['F'], 7):
        es = order[ptr[c]:ptr[c + 1]]
        vs, want = gm[0][es], np.where(sgn[es] > 0, 0.0, 1.0)
        i = b['batch_function_map'][c]
        new = int((~fixed[vs]).sum())
        if np.any(fixed[vs] & (pred[vs] != want)) or (used[i] > 0 and used[i] + new > n_inst[i] // 2):
            continue
        pred[vs], fixed[vs] = want, True
        used[i] += new
    return torch.from_numpy(pred.astype(np.float32))


def loss_run(name, pred, case, dtype, trace=None, keep_edges=None):
    "loss and autograd of the model in ``dtype``: (loss, dpred).  keep_edges: bool [E], the edges of the graph that stay"
    b = batch(name)
    coeff, eps, sharp = LOSS_CASES[case]
    gm, sign = b['gm'], b['sign']
    if keep_edges is not None:
        gm, sign = gm[:, keep_edges], sign[keep_edges]
    x = pred.detach().to(dtype).clone().requires_grad_(True)
    loss = sat_loss(x, gm, sign, b['F'], coeff, eps, sharp, dtype, trace)
    loss.backward()
    return loss.detach(), x.grad


# ---- the error measure -------------------------------------------------------------------------------------------------------------------
def instance_max(x, inst, B):
    "largest x >= 0 per instance (0 for an instance without elements); a NaN stays a NaN"
    return torch.zeros(B, dtype=torch.float64).scatter_reduce(0, inst, x.to(torch.float64), 'amax', include_self=True)


def instance_error(got, ref, inst, B):
    """One workgroup handles one instance, so the error is taken per instance: the largest |got - ref| over the instance's elements over
    the largest |ref| among them, and the maximum of that over the instances (a batch-wide maximum would let a quiet instance hide behind
    a hub's large gradients).  got, ref [n] or [n, c]; inst [n] int64.  An instance whose reference is all zero must be all zero."""
    d = (got.to(torch.float64) - ref.to(torch.float64)).abs().reshape(got.shape[0], -1).amax(1)
    r = ref.to(torch.float64).abs().reshape(ref.shape[0], -1).amax(1)
    dmax, rmax = instance_max(d, inst, B), instance_max(r, inst, B)
    err = torch.where(rmax > 0, dmax / rmax.clamp(min=1e-300), torch.where(dmax > 0, torch.full_like(dmax, float('inf')), dmax))
    return float(err.max())


def bound(err_ref):
    """What a kernel may reach: four times the error of the reference formulation's own fp32 autograd on the same inputs (another, equally
    valid fp32 summation order: ascending edge order here, COO order there), and never less than 4e-6, the figure of this project's
    float64 tests of the GEMM and GRU adjoints."""
    return max(4.0 * err_ref, 4e-6)


# ---- the references, computed once per (batch, case) and shared by the host and the GPU tests -----------------------------------------------
_REF = {}


def sp_reference(name, case):
    """inputs, the float64 and the fp32 run of the model with their clamp decisions, and err_ref per compared gradient: 'dxlog', 'deta_in',
    and 'dy' = deta_in (1 - eta_in), the gradient with respect to log(1 - eta_in) -- on an edge just below 1 the divisor 6e-8 turns the
    fp32 rounding of a row sum minus its own term (6e-8 absolute) into an error of the size of deta_in itself, in the reference's autograd
    as in any fp32 code, so err_ref of deta_in is 0.2 to 0.6 in the clamp cases and the bound on it says little; 'dy' is the same quantity
    before that division and is held to the same rule."""
    if (name, case) not in _REF:
        b, inp = batch(name), sp_inputs(name, case)
        t32, t64 = {}, {}
        r32, r64 = sp_run(name, inp, torch.float32, t32), sp_run(name, inp, torch.float64, t64)
        B = int(b['var_inst'].max()) + 1
        om = 1 - inp['eta_in'].double()
        err = dict(dxlog=instance_error(r32[2], r64[2], b['edge_inst'], B), deta_in=instance_error(r32[3], r64[3], b['edge_inst'], B),
                   dy=instance_error(r32[3].double() * om, r64[3] * om, b['edge_inst'], B))
        _REF[(name, case)] = dict(inp=inp, f32=r32, f64=r64, t32=t32, t64=t64, err_ref=err, om=om, B=B)
    return _REF[(name, case)]


def sp_errors(ref, name, dxlog, deta_in):
    "the three per-instance errors of a kernel's (fp32, CPU) gradients against the float64 model"
    b = batch(name)
    return dict(dxlog=instance_error(dxlog, ref['f64'][2], b['edge_inst'], ref['B']), deta_in=instance_error(deta_in, ref['f64'][3], b['edge_inst'], ref['B']),
                dy=instance_error(deta_in.double() * ref['om'], ref['f64'][3] * ref['om'], b['edge_inst'], ref['B']))


def loss_reference(name, case):
    """pred, the float64 and fp32 runs (loss, dpred) with their traces, and err_ref.  For the fp32-semantics cases (eps = 1e-8) err_ref is
    the fp32 model's error against float64 on a copy of the graph without the edges of the clauses that take the nom <= eps clamp -- the
    ones that overflow --, and 'finite' marks the entries of the fp32 gradient that are finite."""
    if (name, 'loss', case) not in _REF:
        b, pred = batch(name), loss_inputs(name)
        B = int(b['var_inst'].max()) + 1
        t32, t64 = {}, {}
        r32, r64 = loss_run(name, pred, case, torch.float32, t32), loss_run(name, pred, case, torch.float64, t64)
        if case in LOSS_CASES_F32:
            keep = ~t64['nom_clamped'][b['gm'][1]]
            k32, k64 = loss_run(name, pred, case, torch.float32, keep_edges=keep), loss_run(name, pred, case, torch.float64, keep_edges=keep)
            err = instance_error(k32[1], k64[1], b['var_inst'], B)
        else:
            err = instance_error(r32[1], r64[1], b['var_inst'], B)
        _REF[(name, 'loss', case)] = dict(pred=pred, f32=r32, f64=r64, t32=t32, t64=t64, err_ref=err, B=B)
    return _REF[(name, 'loss', case)]
