"""Checkpoints deeper than one ballot of the three resumable searches (pdp_exact_count_round, pdp_exact_solve_round,
pdp_exact_nearest_round): 70 disjoint pairs give a tree of 70 decision levels and rows of 5 words, so a checkpoint's second trip of 64
levels, its upper halves and its odd last word are all written.  A caller-made frontier of prefixes of one 70-level path, one cube per
copy of the instance, runs one round; every record, every checkpoint word and every word of the expanded frontier equals the Python
models (tests/exact_*_rounds_model.py) byte for byte.  What the inputs are meant to reach is checked on the models alone first."""
import faulthandler
import math

import pytest
import torch

import exact_count_rounds_model as cm
import exact_nearest_rounds_model as nm
import exact_solve_rounds_model as sm
import test_exact_count_rounds_gpu as cr
import test_exact_nearest_rounds_gpu as nr
import test_exact_solve_rounds_gpu as sr

PAIRS = 70
INSTANCE = (2 * PAIRS, [[2 * i + 1, 2 * i + 2] for i in range(PAIRS)])
OTHER = {1, 32, 33, 64, 65, 70}                 # levels on their other polarity: the pair (1, 1)
SPENT = {2, 31, 34, 63, 66}                     # levels on their first polarity with nothing owed: the pair (0, 1)
PATH = [(1, 1) if L in OTHER else ((0, 1) if L in SPENT else (0, 0)) for L in range(1, PAIRS + 1)]
PREFIXES = (0, 31, 32, 33, 63, 64, 65, 66, 69)
ROUNDS = [(1, 0), (400, 0), (1, 2)]             # reads per cube, levels given away: the last one expands a deep checkpoint
STEP_LIMIT = 240        # seconds per test: a cube kernel that does not end is a hang, and ends the run with every thread's traceback


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def cubes(full):
    "the frontier's paths: the prefixes, and the whole path for the searches that leave a checkpoint from it"
    return [PATH[:L] for L in PREFIXES + ((PAIRS,) if full else ())]


def marked(path, above=64):
    "the levels past ``above`` whose pair is not (0, 0)"
    return {L for L, pair in enumerate(path, 1) if L > above and pair != (0, 0)}


def two_powers(x):
    "x is 0 or a sum of at most two powers of two: no addition that made it was rounded"
    m, _ = math.frexp(x)
    return bin(int(m * 2.0 ** 53)).count('1') <= 2


def test_the_inputs_reach_what_they_are_meant_to():
    n, clauses = INSTANCE
    assert cm.words(n) == 5 and len(PATH) == PAIRS
    runs = {'count': lambda path, budget: cm.cube(n, clauses, path, budget),
            'solve': lambda path, budget: sm.cube(n, clauses, None, path, budget),
            'nearest': lambda path, budget: nm.cube(n, clauses, None, None, path, budget, None)}
    for name, run in runs.items():
        for L in PREFIXES:
            out = run(PATH[:L], 1)
            assert out[0] == -1 and len(out[-1]) == L + 1 and out[-1][:L] == PATH[:L], (name, L)
    assert [marked(PATH[:L]) for L in (65, 66, 69)] == [{65}, {65, 66}, {65, 66}]
    for name in ('count', 'nearest'):
        out = runs[name](PATH, 1)
        assert out[0] == -1 and len(out[-1]) == PAIRS - 1 and marked(out[-1]) == {65, 66, 69}, name
    done = runs['solve'](PATH, 1)
    assert done[0] == 1 and done[-1] is None                    # the whole path is a model: no checkpoint, so the prefixes only
    for budget in (1, 400):
        assert all(two_powers(runs['count'](path, budget)[1]) for path in cubes(True))


def frontier(state, paths):
    "one cube per instance: the state's root frontier with the rows of ``paths``"
    ln, bits, closed = cm.pack(paths, state.bits.size(1))
    assert state.cubes == len(paths) and state.bits.size(1) == 5
    state.len, state.bits, state.closed = torch.from_numpy(ln).cuda(), torch.from_numpy(bits).cuda(), torch.from_numpy(closed).cuda()
    return state


@pytest.fixture(scope='module')
def problems():
    "one problem of ten copies of the instance, and one of nine"
    return {full: cr.problem([INSTANCE] * len(cubes(full))) for full in (True, False)}


@pytest.mark.gpu
@pytest.mark.parametrize('budget,give', ROUNDS)
def test_count_round_on_deep_paths(problems, budget, give):
    paths = cubes(True)
    inst, p = [INSTANCE] * len(paths), problems[True]
    state, mstate = frontier(p.exact_count_begin(), paths), cm.State(inst)
    mstate.paths = [[path] for path in paths]
    made, rec = cr.one_round(p, state, budget, give)
    want, after = cr.model_round(inst, mstate, budget, give, 5)
    cr.same(rec, want, 'records')
    cr.same(cr.snapshot(state), after, 'state after the round')
    assert made == mstate.cubes() and (budget > 1 or rec['len_out'].max() == PAIRS)


@pytest.mark.gpu
@pytest.mark.parametrize('budget,give', ROUNDS)
def test_solve_round_on_deep_paths(problems, budget, give):
    paths = cubes(False)
    inst, p = [INSTANCE] * len(paths), problems[False]
    state, mstate = frontier(p.exact_solve_begin(), paths), sm.State(inst)
    mstate.paths = [[path] for path in paths]
    made, rec = sr.one_round(p, state, budget, give)
    want, after = sr.model_round(inst, mstate, budget, give, 5)
    sr.same(rec, want, 'records')
    sr.same(sr.snapshot(state), after, 'state after the round')
    assert made == mstate.cubes() and (budget > 1 or rec['len_out'].max() == PAIRS)


@pytest.mark.gpu
@pytest.mark.parametrize('budget,give', ROUNDS)
def test_nearest_round_on_deep_paths(problems, budget, give):
    paths = cubes(True)
    inst, p = [INSTANCE] * len(paths), problems[True]
    state, mstate = frontier(nr.begin(p, inst, None, None, None), paths), nm.State(inst)
    mstate.paths = [[path] for path in paths]
    made, rec = nr.one_round(p, state, budget, give)
    want, after, _ = nr.model_round(inst, mstate, budget, give, 5)
    nr.same(rec, want, 'records')
    nr.same(nr.snapshot(state), after, 'state after the round')
    assert made == mstate.cubes() and (budget > 1 or rec['len_out'].max() == PAIRS)
