"""The three complete searches on the GPU (pdp_exact_solve, pdp_exact_solve_hinted, pdp_exact_solve_learn) past one wave's width:
status, model, work, learned clauses and reductions equal to the Python models (tests/exact_model.py, tests/exact_learn_model.py) on
the instances of tests/exact_wide.py, whose statistics test_exact_wide_host.py asserts -- more than 64 units in a pass, trails past 128,
more than 64 entries undone, analyses that step to the next window of trail slots, clauses of more than 64 literals in the analysis, the
learned clause and a reduction's copy, more than 64 live clauses in a reduction, ids and hint codes past the first chunk -- on the LDS
route, on the HBM route, on both sides of the routing limit, in both builds of the library."""
import numpy as np
import pytest

import exact_model
import exact_wide as xw
import families
from test_exact_gpu import satisfies
from test_exact_learn_gpu import lsolve, on_lds, problem, same, slab_bytes, split

pytestmark = pytest.mark.gpu

LDS_LIMIT = 48 * 1024
LEARN_BATCHES = ['fan', 'wide-0', 'wide-70', 'wide-100', 'wide-130']
KINDS = [None, 'own', 'nan30']


def plain_slab_bytes(n, m, e):
    "ex_lds_layout of csrc/pdp_exact.hip: 21 bytes per variable, two 4-byte entries more, u16 literals and offsets"
    return (21 * n + 8 + 2 * e + 2 * (m + 1) + 15) & ~15


def plain_on_lds(inst):
    n, c = inst
    e = sum(len(x) for x in c)
    n = max([n] + [abs(l) for x in c for l in x])
    return plain_slab_bytes(n, len(c), e) <= LDS_LIMIT and n < 32768 and e <= 65535


def padded(inst, n):
    assert all(k <= n for k in xw.sizes(inst))
    return [(n, c) for _, c in inst]


def leading(got, want):
    "the outputs of instances padded with variables without an occurrence: the unpadded ones, and 0 for the padding"
    for g, w in zip((got[0],) + got[2:], (want[0],) + want[2:]):
        if g is not None:
            np.testing.assert_array_equal(g, w)
    for g, w in zip(got[1], want[1]):
        assert np.array_equal(g[:len(w)], w) and not g[len(w):].any()


def same_plain(got, want):
    "status, work and every model of the plain or hinted search"
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[2])
    assert all(np.array_equal(p, q) for p, q in zip(got[1], want[1]))


def models_hold(inst, got):
    assert all(satisfies(c, m) if s == 1 else not m.any() for (n, c), s, m in zip(inst, got[0], got[1]))


@pytest.mark.parametrize('name', LEARN_BATCHES)
def test_learning_search_on_the_lds_route(name):
    inst, arena, budget = xw.learn_batches()[name]
    want, _ = xw.learn_results(name)
    assert all(on_lds(i, arena) for i in inst)
    got = lsolve(inst, budget=budget, arena=arena)
    same(got, want)
    models_hold(inst, got)
    if budget:
        assert (got[2] < budget + 4 * (xw.edges(inst) + arena)).all() and (got[0] == -1).any()
    if arena:
        assert got[4].any()


@pytest.mark.parametrize('name', LEARN_BATCHES)
def test_learning_search_on_the_hbm_route(name):
    "the same clauses over LEARN_PAD_N variables: no slab fits, the arenas are HBM blocks; the outputs are the unpadded model's"
    inst, arena, budget = xw.learn_batches()[name]
    want, _ = xw.learn_results(name)
    big = padded(inst, xw.LEARN_PAD_N)
    assert not any(on_lds(i, arena) for i in big)
    got = lsolve(big, budget=budget, arena=arena)
    leading(got, want)
    models_hold(big, got)


def hints_for(kind, n=None):
    "the hints of plain_batch(); n: padded to n variables"
    if kind is None:
        return None
    h = xw.plain_hints()[kind]
    return h if n is None else xw.pad_hints(h, n)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('route', ['lds', 'hbm'])
def test_plain_and_hinted_search(route, kind):
    inst = xw.plain_batch()
    want, _ = xw.plain_results(kind)
    if route == 'lds':
        assert all(plain_on_lds(i) for i in inst)
        got = lsolve(inst, hints=hints_for(kind), budget=xw.PLAIN_BUDGET, learn=False)
        same_plain(got, want)
    else:
        big = padded(inst, xw.PLAIN_PAD_N)
        assert not any(plain_on_lds(i) for i in big)
        got = lsolve(big, hints=hints_for(kind, xw.PLAIN_PAD_N), budget=xw.PLAIN_BUDGET, learn=False)
        leading(got, want)
    models_hold(inst, got)
    assert (got[2] < xw.PLAIN_BUDGET + 3 * xw.edges(inst)).all() and (got[0] == -1).any()
    if kind == 'own':
        check_pass_accepts(inst, got, xw.plain_hints()['own'])


def check_pass_accepts(inst, got, hints):
    "hints that satisfy an instance are its model, for the reads of one pass over its clauses"
    ok = [i for i, ((_, c), h) in enumerate(zip(inst, hints)) if exact_model.check_reads(c, h)[1]]
    assert len(ok) >= 20
    for i in ok:
        assert got[0][i] == 1 and got[2][i] == exact_model.check_reads(inst[i][1], hints[i])[0] and np.array_equal(got[1][i][:len(hints[i])], hints[i])
        assert got[3] is None or got[3][i] == 0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('route', ['mixed', 'hbm'])
def test_learning_search_with_hints(route, kind):
    "the instances and hints of the plain search at the default arena: the strided fans are past the learning slab, the others on the LDS route"
    inst = xw.plain_batch()
    want, _ = xw.plain_learn_results(kind)
    e = xw.edges(inst)
    if route == 'mixed':
        far = [i for i, x in enumerate(inst) if not on_lds(x, 0)]
        assert [inst[i] for i in far] == [families.stride(families.fan(100, s), xw.STRIDE) for s in (0, 3)]
        got = lsolve(inst, hints=hints_for(kind), budget=xw.PLAIN_BUDGET)
        same(got, want)
    else:
        big = padded(inst, xw.PLAIN_PAD_N)
        assert not any(on_lds(i, 0) for i in big)
        got = lsolve(big, hints=hints_for(kind, xw.PLAIN_PAD_N), budget=xw.PLAIN_BUDGET)
        leading(got, want)
    models_hold(inst, got)
    assert (got[2] < xw.PLAIN_BUDGET + 4 * (e + 4 * e)).all()
    if kind == 'own':
        check_pass_accepts(inst, got, xw.plain_hints()['own'])


def at_the_limit(inst, per_variable, fixed):
    "the instance with as many variables as make its slab the 48 KiB of the LDS route, and with one more"
    n = (LDS_LIMIT - fixed) // per_variable
    assert n >= xw.sizes([inst])[0]
    return (n, inst[1]), (n + 1, inst[1])


def test_learning_search_on_both_sides_of_the_routing_limit():
    "wide(100), wide_kept(100) and fan(120, 4) at 304 arena words: a slab of exactly 49 152 bytes runs from LDS, one variable more from HBM"
    arena = xw.small_arena(100)
    base = [families.wide(100), families.wide_kept(100), families.fan(120, 4)]
    want, stats = xw.learn_model(xw.interleave(base[:2], base[2:]), arena, xw.FAN_BUDGET)
    assert xw.peak(stats, 'kept_len') == 100 and xw.peak(stats, 'pass_units') == 100 and want[4].max() > 1        # the fan's arena is reduced again and again
    fit, past = [], []
    for inst in base:
        m, e = len(inst[1]), int(xw.edges([inst])[0])
        a, b = at_the_limit(inst, 37, 4 + 2 * (e + arena) + 2 * (m + 1))
        assert slab_bytes(a[0], m, e, arena) == LDS_LIMIT < slab_bytes(b[0], m, e, arena) <= LDS_LIMIT + 48
        assert on_lds(a, arena) and not on_lds(b, arena)
        fit.append(a)
        past.append(b)
    lds = lsolve(xw.interleave(fit[:2], fit[2:]), budget=xw.FAN_BUDGET, arena=arena)
    hbm = lsolve(xw.interleave(past[:2], past[2:]), budget=xw.FAN_BUDGET, arena=arena)
    leading(lds, want)
    leading(hbm, want)
    assert all(np.array_equal(p[:len(q)], q[:len(p)]) for p, q in zip(lds[1], hbm[1]))


@pytest.mark.parametrize('kind', [None, 'nan30'])
def test_plain_search_on_both_sides_of_the_routing_limit(kind):
    "wide(100) and fan(100, 0) under the plain layout (21 n + 8 + 2 e + 2 (m + 1) bytes), without hints and with hints in later chunks"
    inst = xw.plain_batch()
    res, _ = xw.plain_results(kind)
    at = [inst.index(families.wide(100)), inst.index(families.fan(100, 0))]
    few = list(range(3)) + list(range(len(inst) - 3, len(inst)))
    want = tuple([x[i] for i in few[:3] + at + few[3:]] for x in res)
    fit, past = [], []
    for i in at:
        m, e = len(inst[i][1]), int(xw.edges([inst[i]])[0])
        a, b = at_the_limit(inst[i], 21, 8 + 2 * e + 2 * (m + 1))
        assert plain_slab_bytes(a[0], m, e) == LDS_LIMIT < plain_slab_bytes(b[0], m, e) <= LDS_LIMIT + 32
        assert plain_on_lds(a) and not plain_on_lds(b)
        fit.append(a)
        past.append(b)
    runs = []
    for wide in (fit, past):
        batch = [inst[i] for i in few[:3]] + wide + [inst[i] for i in few[3:]]
        hints = None
        if kind:
            picked = [xw.plain_hints()[kind][i] for i in few[:3] + at + few[3:]]
            hints = [xw.pad_hints([h], n)[0] for h, (n, _) in zip(picked, batch)]
        runs.append(lsolve(batch, hints=hints, budget=xw.PLAIN_BUDGET, learn=False))
        leading(runs[-1], want)
    assert all(np.array_equal(p[:len(q)], q[:len(p)]) for p, q in zip(runs[0][1], runs[1][1]))


def test_deterministic_and_instance_local():
    "the 'fan' batch twice on one problem; wide instances alone and inside a batch; both builds of the library"
    from pdp import native
    inst, arena, budget = xw.learn_batches()['fan']
    want, _ = xw.learn_results('fan')
    p = problem(inst)
    a = [t.cpu().numpy() for t in p.exact_solve(budget, learn=True, arena=arena, stats=True)] + [p.exact_learn_reductions().cpu().numpy()]
    b = [t.cpu().numpy() for t in p.exact_solve(budget, learn=True, arena=arena, stats=True)] + [p.exact_learn_reductions().cpu().numpy()]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    same((a[0], split(inst, a[1]), a[2], a[3], a[4]), want)
    del p
    for probe in (inst.index(families.wide(130)), inst.index(families.far_uip(100)), inst.index(families.stride(families.fan(120, 4), xw.STRIDE))):
        one = lsolve([inst[probe]], budget=budget, arena=arena)
        same(one, tuple(x[probe:probe + 1] for x in want))
    D = 100
    kinst, karena, _ = xw.learn_batches()['wide-%d' % D]
    kwant, _ = xw.learn_results('wide-%d' % D)
    probe = kinst.index(families.wide_kept(D))
    same(lsolve([kinst[probe]], arena=karena), tuple(x[probe:probe + 1] for x in kwant))
    prev = native.use_build('fast')
    try:
        fast = lsolve(inst, budget=budget, arena=arena), lsolve(kinst, arena=karena)
        plain = lsolve(xw.plain_batch(), hints=xw.plain_hints()['nan30'], budget=xw.PLAIN_BUDGET, learn=False)
    finally:
        native.use_build(prev)
    same(fast[0], want)
    same(fast[1], kwant)
    same_plain(plain, xw.plain_results('nan30')[0])
