"""E2 of the LDS-resident solver runs without the edge mask in the waves whose slots all have their mask bit (a wave-uniform flag formed
when the record is loaded and at every mask refresh) and with it elsewhere; PDP_SOLVE_NO_CLEAN_TRIPS=1 keeps the mask in every sweep that
has one.  The hazard is a stale flag: a wave that goes on without the mask after a decimation cleared one of its bits, in the same launch or
in the next one.  So the cases are picked from the oracle's trajectory -- instances that never lose a bit, instances that come with cleared
bits, a first decimation in the middle of a launch, in the last sweep of a launch, two in consecutive sweeps -- at the smallest shape with
several trips per wave and a ragged last one (n = 100, m = 420: 1 260 slots, three trips of 512 threads or five of 256), and every case
runs with and without the switch and is compared with the oracle's loop by array_equal: q, fs, edge mask, solution, active masks, executed
sweeps.  What a case needs of the trajectory is asserted, never skipped."""
import numpy as np
import pytest

import families
from helpers import random_batch, load_golden
import test_solve_row_exp_gpu as row_exp
from test_solve_row_exp_gpu import solve_and_compare, oracle_forward, decimation_events

pytestmark = pytest.mark.gpu

SHAPE = dict(batch=64, n=100, k=3, m=420, seed=100)
TOL = 0.05
SWITCH = [False, True]
THREADS = [None, '256']


def _env(monkeypatch, switch, threads=None, **more):
    if switch:
        monkeypatch.setenv('PDP_SOLVE_NO_CLEAN_TRIPS', '1')
    if threads:
        monkeypatch.setenv('PDP_SOLVE_LDS_THREADS', threads)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


_REF = {}


def reference(oracle, T, t_max):
    "the oracle's run of the shared batch, computed once per (T, t_max) and never modified"
    if 'b' not in _REF:
        _REF['b'] = random_batch(**SHAPE)
    if (T, t_max) not in _REF:
        _REF[(T, t_max)] = oracle_forward(oracle, _REF['b'], T, TOL, t_max)
    return _REF['b'], _REF[(T, t_max)]


def lost_slots(b, res):
    "[sweep][instance]: edges whose mask is 0 behind that sweep of the oracle's run (what the next sweep propagates under)"
    ev, ec = b['graph_map'][0].astype(np.int64), b['graph_map'][1].astype(np.int64)
    inst = b['batch_variable_map'].astype(np.int64)[ev]
    B = int(b['batch_variable_map'].max()) + 1
    out = []
    for s in range(res['iterations_run']):
        em = (res['trace_active_var'][s][ev] == 1) & (res['trace_active_fn'][s][ec] == 1)
        out.append(np.bincount(inst[~em], minlength=B))
    return np.array(out)


def refresh_sweeps(lost, i):
    "sweeps of the oracle's run in which instance i lost mask bits (a decimation that fixed something)"
    return [s for s in range(1, lost.shape[0]) if lost[s][i] != lost[s - 1][i]]


# ---- no decimation: the flags never change ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threads', THREADS)
@pytest.mark.parametrize('switch', SWITCH)
def test_instances_that_keep_every_mask_bit(oracle, monkeypatch, switch, threads):
    """t_max = 8 forces the first decimation in the tenth sweep: nine sweeps end before it.  The instances in which simplify() fixed nothing
    keep an all-ones mask throughout -- every wave of theirs runs mask-free in every sweep, the ragged last trip included"""
    _env(monkeypatch, switch, threads)
    b, ref = reference(oracle, 9, 8)
    lost = lost_slots(b, ref[1])
    assert ref[1]['iterations_run'] == 9 and (lost == lost[0]).all()
    assert (lost[0] == 0).sum() * 4 >= lost.shape[1]
    solve_and_compare(oracle, b, 9, TOL, 8, ref=ref)


@pytest.mark.parametrize('threads', THREADS)
@pytest.mark.parametrize('switch', SWITCH)
def test_instances_with_a_pure_literal_at_entry(oracle, monkeypatch, switch, threads):
    """the other instances of the same batch: simplify() peeled pure literals, their records come with cleared bits and the waves that hold
    those slots are masked from the second sweep on (the first runs before the problem has an edge mask), beside waves that are not"""
    _env(monkeypatch, switch, threads)
    b, ref = reference(oracle, 9, 8)
    lost = lost_slots(b, ref[1])
    masked = lost[0] > 0
    assert masked.sum() * 4 >= lost.shape[1] and (~masked).sum() * 4 >= lost.shape[1]
    # cleared slots are a small part of an instance: some 64-slot trips of it stay clean
    E = b['graph_map'].shape[1] // lost.shape[1]
    assert 0 < lost[0][masked].min() and lost[0][masked].max() < E // 4
    solve_and_compare(oracle, b, 9, TOL, 8, ref=ref)


# ---- decimations: a flag falls inside a launch, at its end, twice in a row ----------------------------------------------------------------
@pytest.mark.parametrize('threads', THREADS)
@pytest.mark.parametrize('switch', SWITCH)
def test_decimation_in_the_middle_of_a_launch(oracle, monkeypatch, switch, threads):
    "an instance with an all-ones mask is decimated in the tenth of sixty sweeps (the first launch has fifty): clean -> masked inside one launch"
    _env(monkeypatch, switch, threads)
    b, ref = reference(oracle, 60, 8)
    lost = lost_slots(b, ref[1])
    first = [refresh_sweeps(lost, i)[:1] for i in range(lost.shape[1]) if lost[0][i] == 0]
    assert first and all(f == [9] for f in first)
    assert any(k == 'fast' for s, i, k in decimation_events(b, ref[1]) if s == 9)
    assert ref[1]['iterations_run'] == 60 and not np.isnan(ref[1]['fs']).any()
    solve_and_compare(oracle, b, 60, TOL, 8, ref=ref)


@pytest.mark.parametrize('threads', THREADS)
@pytest.mark.parametrize('switch', SWITCH)
def test_decimation_in_the_last_sweep_of_a_launch(oracle, monkeypatch, switch, threads):
    """PDP_SOLVE_CHUNK=3 makes launches of 6, 3, 3, ... sweeps; with t_max = 7 the first decimation of every instance is in sweep 8, the last
    of the second launch: the refreshed bits reach the third launch through the record, which forms its flags from them"""
    _env(monkeypatch, switch, threads, PDP_SOLVE_CHUNK='3')
    b, ref = reference(oracle, 20, 7)
    lost = lost_slots(b, ref[1])
    first = [refresh_sweeps(lost, i)[:1] for i in range(lost.shape[1]) if lost[0][i] == 0]
    assert first and all(f == [8] for f in first) and 8 % 3 == 2 and 8 >= 5
    assert ref[1]['iterations_run'] == 20
    solve_and_compare(oracle, b, 20, TOL, 7, ref=ref)


@pytest.mark.parametrize('threads', THREADS)
@pytest.mark.parametrize('switch', SWITCH)
def test_two_refreshes_in_consecutive_sweeps(oracle, monkeypatch, switch, threads):
    "instances that are decimated in two and in three sweeps running: a refresh directly behind a refresh, with and without a launch boundary near"
    _env(monkeypatch, switch, threads, **({'PDP_SOLVE_CHUNK': '7'} if threads else {}))
    b, ref = reference(oracle, 60, 8)
    lost = lost_slots(b, ref[1])
    runs = [sum(1 for s in ss if s + 1 in ss) for ss in (refresh_sweeps(lost, i) for i in range(lost.shape[1]))]
    assert sum(1 for r in runs if r >= 1) >= 8 and max(runs) >= 2, runs
    solve_and_compare(oracle, b, 60, TOL, 8, ref=ref)


# ---- other shapes and routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('switch', SWITCH)
def test_structured_family(oracle, monkeypatch, switch):
    "community structure: instances of different sizes in one batch, rows of very different length, decimations of every kind"
    _env(monkeypatch, switch)
    b = families.batch('community-modular')
    if 'community' not in _REF:
        _REF['community'] = oracle_forward(oracle, b, 40, TOL, 8)
    ref = _REF['community']
    assert (ref[1]['trace_active_var'][ref[1]['iterations_run'] - 1] == 0).sum() > 0
    solve_and_compare(oracle, b, 40, TOL, 8, ref=ref)


@pytest.mark.parametrize('adopt', [True, False])
@pytest.mark.parametrize('switch', SWITCH)
def test_poisoned_batch_and_its_replay(oracle, monkeypatch, switch, adopt):
    "the golden poisoned batch of the headline family: NaN surveys go through the unmasked body bit for bit, in pass 1 and in the replay pass"
    from pdp.factorgraph import dataset
    _env(monkeypatch, switch, **({} if adopt else {'PDP_SOLVE_NO_ADOPT': '1'}))
    d = load_golden('headline_n200_poison')
    n, mcl, T = [int(x) for x in d['meta'][:3]]
    items = []
    for sd in d['seeds']:
        items += dataset.random_ksat_items(1, n, 3, m=mcl, seed=int(sd))
    b = dataset.collate_segment(items)
    if 'poison' not in _REF:
        _REF['poison'] = oracle_forward(oracle, b, T, 0.02, 100)
    ref = _REF['poison']
    assert np.isnan(ref[1]['fs']).any() and families.first_nan_sweep(ref[1]) > 0
    hp, _ = solve_and_compare(oracle, b, T, 0.02, 100, ref=ref)
    if not adopt:
        assert hp.last_solve_stats['replays'] >= 1


@pytest.mark.parametrize('switch', SWITCH)
def test_isolated_instances(oracle, monkeypatch, switch):
    "isolate_instances=True: the whole loop in one launch, every refresh of the call inside it"
    _env(monkeypatch, switch)
    b, ref = reference(oracle, 60, 8)
    assert not np.isnan(ref[1]['fs']).any()
    solve_and_compare(oracle, b, 60, TOL, 8, ref=ref, isolated=True)


@pytest.mark.parametrize('switch', SWITCH)
def test_forced_and_reinforce_instantiations(oracle, monkeypatch, switch):
    "the Reinforce triple and p-d-p with a caller's force column keep the masked body everywhere: still the oracle's results, switch or not"
    _env(monkeypatch, switch)
    row_exp.test_forced_and_reinforce_forward_unchanged(oracle)
