"""pdp_exact_nearest relaunched on one handle between the other complete searches, in the manner of tests/exact_reuse.py: the cached
routing, the instance order, the counter and the HBM working arrays of a handle are shared by all of them, and with PDP_EXACT_GRID=1 one
wave runs the whole batch in one slab, every instance over what its predecessor -- of this search or of another -- left there.  The
answers stay the Python statement's (tests/exact_nearest_model.py) whatever ran before, and the other searches' answers do not move."""
import faulthandler
import functools

import numpy as np
import pytest

import exact_nearest_cases as cs
import exact_nearest_model as nm
import exact_reuse as xr
import exact_wide as xw
from test_exact_nearest_gpu import flat, problem, run

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def limit():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def dressed(inst, seed):
    inst = [(n, c) for n, (_, c) in zip(xw.sizes(inst), inst)]
    rng = np.random.RandomState(seed)
    hints = [rng.randint(0, 2, size=n).astype(np.float32) for n, _ in inst]
    return inst, hints, [cs.penalties_of(rng, n) for n, _ in inst]


@functools.lru_cache(maxsize=None)
def crossing():
    "crossing(): literal counts fall while variable counts rise, so every array of a successor lies over other arrays of its predecessor"
    inst, hints, pens = dressed(xr.crossing(), 4500)
    return inst, hints, pens, nm.solve(inst, hints, pens, xr.CROSS_BUDGET)


@functools.lru_cache(maxsize=None)
def routes():
    "routes(): HBM-routed and LDS-routed instances alternate in one batch"
    inst, hints, pens = dressed(xr.routes()[0], 4600)
    return inst, hints, pens, nm.solve(inst, hints, pens, xr.ROUTES_BUDGET)


def others(p, inst, hints):
    "what the other searches of the handle answer, as numpy"
    h = flat(p, inst, hints, np.float32, 0.0)
    out = [p.exact_solve(xr.CROSS_BUDGET), p.exact_solve(xr.CROSS_BUDGET, hints=h), p.exact_min_unsat(xr.CROSS_BUDGET, hints=h),
           p.exact_count(xr.CROSS_BUDGET)]
    return [[t.cpu().numpy() for t in r] for r in out]


@pytest.mark.parametrize('grid', ['1', None])
def test_nearest_between_the_other_searches_of_one_handle(grid, monkeypatch):
    inst, hints, pens, want = crossing()
    assert (want[0] == -1).any() and (want[0] == 1).any() and (want[4] > 0).any()
    if grid:
        monkeypatch.setenv('PDP_EXACT_GRID', grid)
    p = problem(inst)
    cs.same(run(inst, hints, pens, xr.CROSS_BUDGET, prob=p), want)                         # the first call of the handle: it prepares the routing
    before = others(p, inst, hints)
    cs.same(run(inst, hints, pens, xr.CROSS_BUDGET, prob=p), want)                         # behind four other searches
    after = others(p, inst, hints)                                                      # and they behind it
    for a, b in zip(before, after):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    q = problem(inst)
    fresh = others(q, inst, hints)                                                      # a handle that never ran the nearest-model search
    for a, b in zip(before, fresh):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    cs.same(run(inst, hints, pens, xr.CROSS_BUDGET, prob=q), want)
    if grid:
        assert p.exact_last_grid() == 1


def test_nearest_on_both_routes_of_one_handle(monkeypatch):
    inst, hints, pens, want = routes()
    monkeypatch.setenv('PDP_EXACT_GRID', '1')
    p = problem(inst)
    h = flat(p, inst, hints, np.float32, 0.0)
    first = [t.cpu().numpy() for t in p.exact_solve(xr.ROUTES_BUDGET, hints=h)]
    cs.same(run(inst, hints, pens, xr.ROUTES_BUDGET, prob=p), want)
    p.exact_count(xr.ROUTES_BUDGET)
    cs.same(run(inst, hints, pens, xr.ROUTES_BUDGET, prob=p), want)
    again = [t.cpu().numpy() for t in p.exact_solve(xr.ROUTES_BUDGET, hints=h)]
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    assert p.exact_last_grid() == 1
