"""The structured instance families of tests/families.py, checked without a GPU: each generator is deterministic and delivers the
structure it promises, and the CPU oracle's runs on every family batch meet the conditions that keep the GPU comparison of
tests/test_families_gpu.py from being vacuous (variables stay active after simplify, sweeps run NaN-free before a poison, Walk-SAT
flips, both answers occur in the complete solver's ground truth)."""
import numpy as np
import pytest

import families
from test_exact_host import brute_force, dpll


def _problem(oracle, b):
    return oracle.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])


@pytest.fixture(scope='module')
def batches():
    return {name: families.batch(name) for name in families.NAMES}


def test_generators_are_deterministic(batches):
    for name in families.NAMES:
        again = families.batch(name)
        for key in ('graph_map', 'batch_variable_map', 'batch_function_map', 'edge_feature'):
            np.testing.assert_array_equal(batches[name][key], again[key], err_msg=name)
    a, b = families.exact_cases(), families.exact_cases()
    assert a == b
    # another seed gives another instance
    assert families.hub(np.random.RandomState(1), 16) != families.hub(np.random.RandomState(2), 16)
    assert families.regular(np.random.RandomState(1), 4, 3, 300) != families.regular(np.random.RandomState(2), 4, 3, 300)


def test_batches_hold_4_to_64_instances_of_one_family(oracle, batches):
    for name in families.NAMES:
        assert 4 <= len(families.table(batches[name])) <= 64, name
        # some variable is inactive after simplify (the anchor's, or a solved chain): the exact zero a speculative resident run counts on
        op = _problem(oracle, batches[name])
        op.simplify()
        assert op.state()[0].min() == 0.0, name
    # every d, k, position and size the families are made for is there
    assert {d for nm in families.NAMES if nm.startswith('hub-') for d in map(int, nm.split('-')[1:])} == \
        {15, 16, 17, 31, 32, 33, 64, 128, 254, 255, 256, 257, 1000, 3000}
    assert {int(nm.split('-')[1]) for nm in families.NAMES if nm.startswith('long-') and 'only' not in nm} == {63, 64, 65, 255, 256, 257, 1000}
    sizes = lambda tag: {r['n'] for nm in families.NAMES if nm.startswith(tag) for r in families.table(batches[nm])}  # noqa: E731
    assert all(any(n <= s <= n + 1 for s in sizes('ladder-4.2')) for n in range(100, 701, 20))       # (+ 1: a batch's anchor variable)
    # (at alpha 3 a variable may occur nowhere, and the loader drops it)
    assert all(any(n - 2 <= s <= n + 1 for s in sizes('ladder-3.0')) for n in range(100, 601, 20))


@pytest.mark.parametrize('name', families.NAMES)
def test_stated_properties(batches, name):
    "the structure table computed from the collated batch against the family's promise"
    rows = families.table(batches[name])
    pr = families.promise(name)
    max_deg, max_len = max(r['max_degree'] for r in rows), max(r['max_length'] for r in rows)
    epv = sum(r['e'] for r in rows) / float(sum(r['n'] for r in rows))
    assert max_len == pr['k'], (max_len, pr['k'])
    if 'deg' in pr:
        assert pr['deg'][0] <= max_deg <= pr['deg'][1], max_deg
    if 'epv' in pr:
        assert pr['epv'][0] <= epv <= pr['epv'][1], epv
    fits = [families.fits_lds(r) for r in rows]
    if pr.get('hbm_all'):
        assert not any(fits)
    if pr.get('mixed_routes'):
        assert any(fits) and not all(fits)
    if name.startswith('hub-'):
        # the hub is variable 1 of its instance, and nobody else comes close
        b = batches[name]
        deg = np.bincount(b['graph_map'][0], minlength=b['batch_variable_map'].size)
        first = np.r_[0, np.cumsum([r['n'] for r in rows])[:-1]]
        want = [int(d) for d in name.split('-')[1:]]
        for i, r in enumerate(rows):
            assert deg[first[i]] == r['max_degree'] and any(d <= r['max_degree'] <= d + 30 for d in want + [64, 128])
    if name.startswith('long-') and 'only' not in name:
        # ONE long clause per instance, at the promised position
        b = batches[name]
        length = np.bincount(b['graph_map'][1], minlength=b['batch_function_map'].size)
        first = np.r_[0, np.cumsum([r['m'] for r in rows])[:-1]]
        ats = families.LONG_AT if pr['k'] != 1000 else (0, 64, 255, -1)
        for i, (r, at) in enumerate(zip(rows, ats)):
            seg = length[first[i]:first[i] + r['m']]
            assert (seg == pr['k']).sum() == 1 and (seg == 3).sum() == r['m'] - 1 - (i == 0)      # (the first instance carries the batch's anchor)
            assert int(np.argmax(seg)) == (at if at >= 0 else r['m'] + at)
    if name.startswith('long-only'):
        b = batches[name]
        length = np.bincount(b['graph_map'][1])
        assert (length == pr['k']).sum() == length.size - 1 and length.min() == 1                  # (all but the anchor's unit clause)
    if name.startswith('regular-'):
        # alternating signs: no variable is pure, and (nearly) every variable has the full degree
        b = batches[name]
        V = b['batch_variable_map'].size
        pos = np.bincount(b['graph_map'][0], weights=(b['edge_feature'].reshape(-1) > 0), minlength=V)
        deg = np.bincount(b['graph_map'][0], minlength=V)
        assert (deg == pr['deg'][0]).mean() > 0.9 and ((pos > 0) & (pos < deg)).mean() > 0.99


def test_ladders_cross_the_lds_limit_inside_a_batch(batches):
    "a fitting and a non-fitting neighbour in the same batch, for both densities; the big hub sits next to fitting ones too"
    for tag in ('ladder-4.2', 'ladder-3.0'):
        crossing = []
        for nm in families.NAMES:
            if nm.startswith(tag):
                fits = [families.fits_lds(r) for r in families.table(batches[nm])]
                if any(fits) and not all(fits):
                    crossing.append(nm)
        assert crossing, tag


def test_ladders_cross_the_walksat_and_simplify_limits(batches):
    """Walk-SAT routes per instance (64 KiB): a fitting and a non-fitting neighbour share a batch on both ladders.  Simplify routes per
    batch (64 KiB for its largest sizes): both sides occur on the alpha 4.2 ladder; at alpha 3.0 the largest batch (n = 600) still fits
    with 59 KiB, and PDP_SIMPLIFY_HBM reaches the other form there."""
    for tag in ('ladder-4.2', 'ladder-3.0'):
        ws, simp = set(), set()
        for nm in families.NAMES:
            if nm.startswith(tag):
                rows = families.table(batches[nm])
                fits = [families.walksat_lds_bytes(r['n'], r['m'], r['e']) <= 64 * 1024 for r in rows]
                if any(fits) and not all(fits):
                    ws.add(nm)
                simp.add(families.simplify_lds_bytes(max(r['n'] for r in rows), max(r['m'] for r in rows), max(r['e'] for r in rows)) <= 64 * 1024)
        assert ws and simp == ({True, False} if tag == 'ladder-4.2' else {True}), tag


def test_families_reach_the_launch_forms_of_the_resident_solver(batches):
    """Which family reaches which form of k_sp_solve_lds, from the launch rules (families.solver_launch): the uniform batches of the older
    tests only ever get the register-cached P4 work item and helper waves for the clause rows."""
    from helpers import random_batch
    for spec in (dict(batch=16, n=50, k=3, seed=7), dict(batch=64, n=40, mixed=True, seed=100), dict(batch=6, n=200, k=3, seed=11),
                 dict(batch=3, n=300, k=3, seed=9)):
        L = families.solver_launch(families.table(random_batch(**spec)))
        assert all(L['cached']) and min(L['helpers']) > 0
    launch = {nm: families.solver_launch(families.table(batches[nm])) for nm in families.NAMES}
    want = {'regular-4-2-n130': (256, False, 1), 'regular-4-2-n200': (256, False, 0), 'regular-4-2-n250': (256, False, 0),
            'regular-4-3-n300': (512, False, 3), 'regular-4-3-n600': (1024, False, 6), 'regular-4-3-n900': (1024, False, 1),
            'regular-4-3-n1000': (1024, False, 0), 'regular-6-3-n500': (1024, True, 8), 'regular-6-3-n700': (1024, False, 5)}
    for nm, (nt, cached, helpers) in want.items():
        L = launch[nm]
        assert L['threads'] == nt and set(L['cached']) == {cached} and set(L['helpers']) == {helpers}, (nm, L)
    assert launch['regular-6-3-n800'] is None and launch['long-1000'] is None                 # past the LDS limit: HBM-resident only
    assert launch['regular-4-3-n1000']['image'] > 140 * 1024                                  # u16 slot words at n = 1 000, m = 1 330
    # every thread count the library chooses occurs on hubs, and the uncached form also on the alpha 3.0 ladder from n = 520 on
    assert [launch[nm]['threads'] for nm in ('hub-128', 'hub-254-255-256-257', 'hub-1000')] == [256, 512, 1024]
    assert not any(launch['ladder-3.0-n520-600']['cached'])
    # ... and on a hub of more than 255 edges (the hubs on 60 variables are all cached)
    L = launch['sparsehub-300']
    assert L['threads'] == 1024 and not any(L['cached']) and min(r['max_degree'] for r in families.table(batches['sparsehub-300'])) > 255
    # the thread-count test's headline batch at 256 threads: uncached, no helper wave, on a dense instance
    L = families.solver_launch(families.table(random_batch(batch=6, n=200, k=3, m=840, seed=11)), threads=256)
    assert not any(L['cached']) and set(L['helpers']) == {0}


def test_lds_image_formula_matches_the_library_source():
    "lds_image_bytes mirrors lds2_bytes_for; a change there must be followed here (it decides what the GPU tests expect of used_lds)"
    import os
    import re
    src = open(os.path.join(families.helpers.REPO, 'pdp-solver_amd', 'csrc', 'pdp_solve.hip')).read()
    body = src[src.index('static size_t lds2_bytes_for'):]
    body = body[:body.index('return s;')]
    terms = re.findall(r's \+= (.*?);', body)
    assert terms == ['5 * a16((size_t)e * 4)', '3 * a16((size_t)e * 2)', 'a16((size_t)(n + 1) * 2) + a16((size_t)(m + 1) * 2)',
                     'a16((size_t)(m + 8) * 4) + a16((size_t)m * 4)', '7 * a16((size_t)n * 4)', 'a16((size_t)n)', 'a16((size_t)n * 2)']
    assert 'lds2_bytes_for(n, m, e) <= 160 * 1024 - 1024 && e < 65535 && n < 16384 && m < 16384' in src


@pytest.mark.parametrize('name', families.NAMES)
def test_oracle_conditions(oracle, batches, name):
    """simplify + forward('p-d-p') + forward('reinforce') + Walk-SAT on the oracle alone: at least half of the variables stay active
    after simplify (all families but chains and minimal), and every batch used with pdp_sp_solve has a compared run of >= 5 executed
    NaN-free sweeps -- except the batches the oracle poisons in sweep 1 and the ones it solves at once, which families.py lists by name."""
    b = batches[name]
    op = _problem(oracle, b)
    op.simplify()
    active = op.state()[0]
    if not name.startswith(('chains', 'minimal')):
        assert active.mean() >= 0.5, active.mean()
    else:
        rows = families.table(b)
        first = np.r_[0, np.cumsum([r['n'] for r in rows])]
        if name.startswith('chains'):
            # simplify solves the two chains completely (the point is the number of fix-point rounds), not the ordinary instance
            for i in (0, 2, 3):
                assert active[first[i]:first[i + 1]].sum() == 0
            assert active[first[1]:first[2]].mean() > 0.5
    coins = np.random.RandomState(1).rand(40).astype(np.float32)
    runs = dict(sp=lambda T: _problem(oracle, b).forward('p-d-p', T, local_search_iterations=0, tolerance=0.05, t_max=8, seed=5, trace=True, trace_float=True),
                rf=lambda T: _problem(oracle, b).forward('reinforce', T, local_search_iterations=0, pi=0.1, decimation_probability=0.5,
                                                         stream=coins[:T], trace=True, trace_float=True))
    for model, fwd in runs.items():
        full = fwd(40)
        s = families.first_nan_sweep(full)
        plan = families.sweep_plan(lambda T: full)
        if name in families.POISONED_IN_SWEEP_1:
            assert s == 0 and plan == [40], (model, s)
            continue
        assert s != 0, "poisoned in sweep 1: list the batch in POISONED_IN_SWEEP_1"
        assert plan == ([40] if s is None else [40, s])
        clean = full if s is None else fwd(s)
        assert families.first_nan_sweep(clean) is None and not np.isnan(clean['q']).any() and not np.isnan(clean['fs']).any()
        if name in families.SOLVED_AT_ONCE:
            assert clean['iterations_run'] <= 3
        elif not name.startswith('minimal'):
            assert clean['iterations_run'] >= 5, (model, plan, clean['iterations_run'])
        if s is not None:
            assert np.isnan(full['fs']).any() or np.isnan(full['q']).any()
    # Walk-SAT from a random fill flips something on every batch with active variables
    op.random_fill(seed=1234)
    pred = op.state()[2]
    out, steps, _ = op.local_search(pred, 200, 0.5, seed=99)
    assert 0 <= steps <= 200
    if not name.startswith('minimal') and name not in families.SOLVED_AT_ONCE:
        assert (out != pred).any()


def test_hub_poison_comes_earlier_with_the_degree(oracle, batches):
    "the reference's arithmetic on a hub: no NaN in 40 sweeps up to d = 64, a first NaN that moves forward with d, sweep 1 at d = 1 000"
    first = {}
    for name in ('hub-64', 'hub-128', 'hub-254-255-256-257', 'hub-1000'):
        res = _problem(oracle, batches[name]).forward('p-d-p', 40, local_search_iterations=0, tolerance=0.05, t_max=8, seed=5, trace=True, trace_float=True)
        first[name] = families.first_nan_sweep(res)
    assert first['hub-64'] is None and first['hub-1000'] == 0
    assert 5 <= first['hub-254-255-256-257'] < first['hub-128'] < 40


def test_complete_solver_ground_truth():
    "the answers of the family instances part of the GPU test uses, by the independent DPLL (and the enumerator where it can): both occur"
    cases = families.exact_cases()
    want = [dpll(n, c) for _, n, c in cases]
    for (name, n, c), w in zip(cases, want):
        if n <= 20:
            assert brute_force(n, c) == w, name
    assert sum(want) >= 5 and len(want) - sum(want) >= 5
    for fam in ('hub', 'long', 'regular', 'power', 'minimal', 'ladder'):
        assert any(name.startswith(fam) for name, _, _ in cases)
    # the hard cores of the composed instances
    from test_exact_host import pigeonhole
    assert not dpll(*pigeonhole(5))
    cores = families.threshold_cores()
    answers = [dpll(n, c) for n, c in cores]
    assert True in answers and False in answers


@pytest.mark.parametrize('place', ['first', 'last', 'interleaved'])
def test_compose_is_a_disjoint_union(place):
    core = (3, [[1, 2], [-2, 3], [-1, -3], [2]])
    big = (5, [[1, -5], [2, 3, 4], [-4, 5], [1], [2, -3], [3], [4, 5], [-1, 2]])
    n, clauses, core_ids = families.compose(core, big, place)
    assert n == 8 and len(clauses) == 12 and len(set(core_ids)) == 3
    in_core = [all(abs(l) in set(core_ids) for l in c) for c in clauses]
    in_big = [all(abs(l) not in set(core_ids) for l in c) for c in clauses]
    assert sum(in_core) == 4 and sum(in_big) == 8
    back = {int(v): i + 1 for i, v in enumerate(core_ids)}
    assert [[back[abs(l)] * (1 if l > 0 else -1) for l in c] for c, k in zip(clauses, in_core) if k] == core[1]
    where = [i for i, k in enumerate(in_core) if k]
    assert where == {'first': [0, 1, 2, 3], 'last': [8, 9, 10, 11]}.get(place, where) and (place != 'interleaved' or where[-1] - where[0] > 4)
    assert brute_force(n, clauses) == (brute_force(*core) and brute_force(*big))
