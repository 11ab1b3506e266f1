"""The batches that pin slab reuse and relaunch of the complete solvers (tests/exact_reuse.py), on the CPU: the facts that
test_exact_reuse_gpu.py relies on.  In launch order every instance of crossing() has fewer literals and more variables than the one
before, so its per-variable arrays start over bytes where the predecessor kept literals; every instance is on the route the GPU test
says; most searches meet a conflict; and every outcome of a search -- satisfiable, unsatisfiable, out of budget, out of arena, answered
by the check pass -- occurs in an instance that one wave runs before another one."""
import ctypes
import os

import numpy as np

import exact_model
import exact_reuse as xr
import exact_wide as xw
from test_exact_learn_gpu import on_lds, slab_bytes
from test_exact_proof_gpu import check_cases, check_on_lds
from test_exact_wide_gpu import LEARN_BATCHES, plain_on_lds, plain_slab_bytes

ARENAS = (0, xr.CROSS_ARENA)
FITS = [('plain', plain_on_lds)] + [('learn', lambda x, A=A: on_lds(x, A)) for A in ARENAS] + [('check', check_on_lds)]


def test_layout_formulas_agree_with_the_totals_the_other_tests_state():
    for n, m, e in xr.dims(xr.crossing()) + xr.dims(xr.routes()[0]):
        assert (xr.slab_end('plain', n, m, e) + 15) & ~15 == plain_slab_bytes(n, m, e)
        for A in ARENAS:
            assert (xr.slab_end('learn', n, m, e, A) + 15) & ~15 == slab_bytes(n, m, e, A)
        assert (xr.slab_end('check', n, m, e) + 15) & ~15 == (5 * n + 2 * e + 2 * (m + 1) + 15) & ~15


def test_crossing_falls_in_literals_and_rises_in_variables():
    inst = xr.crossing()
    d = xr.dims(inst)
    assert len(inst) >= 24
    for _, fits in FITS:
        assert xr.launch_order(inst, fits) == list(range(len(inst)))                # the batch is in launch order on every route
    for a, b in zip(d, d[1:]):
        assert b[2] < a[2] and b[0] > a[0]
        for layout in ('plain', 'learn', 'check'):
            for A in (ARENAS if layout == 'learn' else (0,)):
                # the successor's 4-byte arrays: longer than the predecessor's, and the part past them lies over its literals
                assert xr.per_variable_bytes(layout, b[0]) > xr.per_variable_bytes(layout, a[0])
                over = xr.overlaid(layout, a, b, A)
                assert over >= min(2 * a[2], xr.per_variable_bytes(layout, b[0]) - xr.per_variable_bytes(layout, a[0])) > 0
    # from about 10 variables to within one step of the 48 KiB of the learning layout
    last, step = xr.cross_step()
    assert d[0][0] == xr.CROSS_N0 <= 12 and d[-1][0] == last and all(b[0] - a[0] == step for a, b in zip(d, d[1:]))
    n, m, e = d[-1]
    assert slab_bytes(n, m, e, 0) <= xr.LDS_LIMIT < slab_bytes(n + step, m, e, 0)
    assert [c for _, c in inst] == [c for _, c in xr.shrinking()]
    sd = xr.dims(xr.shrinking())
    assert all(b[2] < a[2] for a, b in zip(sd, sd[1:])) and sd[-1][0] < sd[0][0] and not any(b[0] > a[0] + 30 for a, b in zip(sd, sd[1:]))


def test_every_instance_is_on_the_route_the_gpu_test_says():
    mixed, padded = xr.routes()
    hbm = [x for x in mixed if x[0] == xr.PAD_N]
    lds = [x for x in mixed if x[0] != xr.PAD_N]
    assert len(hbm) == len(xr.ROUTES_HBM) >= 8 and len(lds) == len(xr.ROUTES_LDS) >= 16
    for name, fits in FITS + [('learn', lambda x: on_lds(x, xr.ROUTES_ARENA))]:
        assert all(fits(x) for x in xr.crossing() + xr.shrinking() + lds), name
        assert not any(fits(x) for x in hbm + padded), name
        order = xr.launch_order(mixed, fits)
        assert all(mixed[i][0] == xr.PAD_N for i in order[:len(hbm)]) and order != list(range(len(mixed)))
    assert all(plain_on_lds(x) and on_lds(x, 0) and check_on_lds(x) for x in xr.tiny())


def test_most_searches_of_crossing_backtrack():
    half = len(xr.cores()) // 2
    for stats in (xr.cross_plain(False)[1], xr.cross_plain(True)[1]) + tuple(xr.cross_learn(A, h)[1] for A in ARENAS for h in (False, True)):
        assert sum('trail' in s for s in stats) >= half + 1                          # 'trail': the trail's length at a conflict
    assert xr.cross_learn(xr.CROSS_ARENA)[0][4].any() and not xr.cross_learn(0)[0][4].any()          # the reduced arena is reduced
    assert (xr.cross_proof(xr.CROSS_ARENA)[6] > 0).sum() >= half


def answered_by_check(inst, hints, res):
    "instances whose hints are complete and satisfy them: status 1 for the reads of one pass"
    flags = []
    for (_, c), h, s, w in zip(inst, hints, res[0], res[2]):
        ok = not np.isnan(h).any() and exact_model.check_reads(c, h)[1]
        assert not ok or (s == 1 and w == exact_model.check_reads(c, h)[0])
        flags.append(ok)
    return flags


def test_every_outcome_occurs_in_a_predecessor():
    "in launch order, in an instance that is not the last: under PDP_EXACT_GRID=1 the same wave then runs another instance in its slab"
    # crossing() and shrinking(): launch order = batch order
    order = list(range(len(xr.cores())))
    plain, learn = xr.cross_plain(False)[0], xr.cross_learn(xr.CROSS_ARENA)[0]
    for res in (plain, learn, xr.cross_learn(0)[0]):
        assert xr.predecessors(order, res[0] == 1) >= 5, "status 1 as a predecessor"
        assert xr.predecessors(order, res[0] == 0) >= 5, "status 0 as a predecessor"
    assert xr.predecessors(order, (plain[0] == -1) & (plain[2] >= xr.CROSS_BUDGET)) >= 2, "status -1 by budget as a predecessor"
    hinted = xr.cross_plain(True)[0]
    passed = answered_by_check(xr.cores(), xr.cross_hints(), hinted)
    assert xr.predecessors(order, passed) >= 3, "a hinted instance answered by the check pass as a predecessor"
    assert xr.predecessors(order, [not np.isnan(h).any() and not p for h, p in zip(xr.cross_hints(), passed)]) >= 3         # the check pass fails: val is cleared again
    assert xr.predecessors(order, [np.isnan(h).any() for h in xr.cross_hints()]) >= 3
    # the mixed batch: the 12-word arena runs out (no budget: every -1 is the arena's), the plain search runs out of budget
    inst, runs = xr.mixed()
    assert len(inst) == 473
    for A in (0, 12, 40):
        order = xr.launch_order(inst, lambda x: on_lds(x, A))
        assert len(order) == len(inst) and all(on_lds(x, A) for x in inst)
        assert xr.predecessors(order, runs[A][0] == 1) > 100 and xr.predecessors(order, runs[A][0] == 0) > 100
        assert xr.predecessors(order, runs[A][4] > 0) >= (3 if A else 0)            # a reduced arena left behind
    order = xr.launch_order(inst, lambda x: on_lds(x, 12))
    assert xr.predecessors(order, runs[12][0] == -1) >= 3, "status -1 by an exhausted arena as a predecessor"
    order = xr.launch_order(inst, plain_on_lds)
    for kind in (None, 'own', 'nan30'):
        res = xr.mixed_plain(kind)[0]
        assert xr.predecessors(order, (res[0] == -1) & (res[2] >= xr.MIXED_BUDGET)) >= 3, "status -1 by budget as a predecessor"
        assert ((res[0] == -1) == (res[2] >= xr.MIXED_BUDGET)).all()
    own = xr.mixed_plain('own')[0]
    assert xr.predecessors(order, answered_by_check(inst, xr.mixed_hints()['own'], own)) > 100, "answered by the check pass as a predecessor"
    # routes(): every outcome on the HBM route, which a wave runs first, and on the LDS route
    mixed, _ = xr.routes()
    cores = xr.routes_cores()
    for fits, res in ((plain_on_lds, xr.routes_plain(None)[0]), (lambda x: on_lds(x, 0), xr.routes_learn(0)[0]),
                      (lambda x: on_lds(x, xr.ROUTES_ARENA), xr.routes_learn(xr.ROUTES_ARENA)[0])):
        order = xr.launch_order(mixed, fits)
        k = len(xr.ROUTES_HBM)
        for part in (order[:k + 1], order[k:]):                                      # the HBM instances are followed by the first LDS one
            assert xr.predecessors(part, res[0] == 1) >= 2 and xr.predecessors(part, res[0] == 0) >= 2
            assert xr.predecessors(part, (res[0] == -1) & (res[2] >= xr.ROUTES_BUDGET)) >= 1, "status -1 by budget as a predecessor, both routes"
    assert answered_by_check(cores, xr.routes_hints()['own'], xr.routes_plain('own')[0]).count(True) >= 10
    assert xr.routes_learn(xr.ROUTES_ARENA)[0][4].any()
    # the wide batches with their small neighbours
    for name in LEARN_BATCHES:
        binst, arena, budget = xw.learn_batches()[name]
        res = xw.learn_results(name)[0]
        order = xr.launch_order(binst, lambda x: on_lds(x, arena))
        assert xr.predecessors(order, res[0] == 1) >= 3
        small = set(binst.index(x) for part in xw.few() for x in part)
        assert any(a not in small and b in small for a, b in zip(order, order[1:]))  # a small instance right after a wide one
    fan = xw.learn_results('fan')[0]
    assert ((fan[0] == -1) & (fan[2] >= xw.FAN_BUDGET)).sum() >= 2                   # the largest instances: they run first


def test_the_checkers_batches_interleave_every_kind():
    "in the checker's launch order accepted, refuted and unverified instances each precede another one, on both routes"
    from test_exact_proof_gpu import CHECK_PAD_N
    for pad in (0, CHECK_PAD_N):
        batch, status, models, regions, plen, want = check_cases(pad)
        order = xr.launch_order(batch, check_on_lds)
        for v in (1, 0, -1):
            assert xr.predecessors(order, want[0] == v) >= 3
        kinds = [int(want[0][i]) for i in order]
        assert sum(a != b for a, b in zip(kinds, kinds[1:])) >= 20                   # interleaved, not in three runs


def test_tiled_instances():
    t = xr.tiny()
    assert len(t) == xr.TINY == 64 and len({repr(x) for x in t}) == 64
    for n, c in t:
        assert 3 <= n <= 8 and 4 <= len(c) <= 30 and all(1 <= len(x) <= 3 for x in c)
    idx = xr.tiled_index(20000)
    assert np.bincount(idx, minlength=64).min() >= 312 and not np.array_equal(idx, np.arange(20000) % 64)
    assert np.array_equal(idx, xr.tiled_index(20000)) and xr.tiled(130)[:5] == [t[i] for i in xr.tiled_index(130)[:5]]
    r = xr.tiny_results()
    assert {0, 1} == set(r['plain'][0].tolist()) and np.array_equal(r['plain'][0], r['proof'][0])
    assert (r['check'][0] == 1).all() and (r['proof'][6] > 0).sum() >= 8


def test_the_switch_is_declared_and_exported():
    "the header, the symbol list and (test_host_logic.py) their parity; the entry point refuses NULL without touching a device"
    from helpers import REPO
    from pdp import native
    assert 'pdp_exact_last_grid' in native.EXPORTED_SYMBOLS
    header = open(os.path.join(REPO, 'include', 'pdp_hip.h')).read()
    assert 'int pdp_exact_last_grid(const pdp_problem *p, int32_t *grid_host);' in header and 'PDP_EXACT_GRID' in header
    assert hasattr(native.Problem, 'exact_last_grid')
    out = ctypes.c_int32(-7)
    assert native.lib().pdp_exact_last_grid(None, ctypes.byref(out)) == 1 and out.value == -7               # PDP_ERR_INVALID
