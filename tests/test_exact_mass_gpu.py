"""The weighted counting search on the GPU (pdp_exact_mass, Problem.exact_mass, exact.solution_mass, satyr.py --complete
--complete-mass): equal to its Python statement (tests/exact_mass_model.py) bit for bit in status, mass, true_mass, open_mass, work and
leaves, to the counting search at weights 0.5, to exact rational arithmetic at weights that are multiples of 1/8, 0/1 weights, the
budget's bracket, determinism over batch, handle, grid and build, the HBM route, refused instances, refusals, and the command line."""
import ctypes
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_count_cases as cs
import exact_mass_cases as zc
import exact_mass_model as zm
import exact_model
import exact_wide
import families
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
BATCH_BUDGET = 1 << 22
N50_SEED = 53


def problem(inst):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment([exact.raw_item(n, c) for n, c in inst]), torch.device('cuda:0'))
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(inst))


def device_weights(weights):
    return torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.float32) for w in weights])).to('cuda:0')


def run(inst, weights, budget=0, prob=None):
    "the six outputs of Problem.exact_mass in the layout of exact_mass_model.solve"
    p = problem(inst) if prob is None else prob
    st, mass, tm, open_mass, work, leaves = [t.cpu().numpy() for t in p.exact_mass(device_weights(weights), budget, stats=True)]
    ends = np.cumsum([zc.size(i) for i in inst])
    return st, mass, np.split(tm, ends[:-1]), open_mass, work, leaves


def wide_cases():
    """exact_wide's fans (100 units in one pass at level 0, trails past 128) under weights that leave a tree the model can walk: the
    deciding model's assignment as 0/1 weights with every seventh variable soft, and one under 0.9 around it that ends at the budget"""
    inst, weights = [], []
    for k, seed in enumerate(exact_wide.PLAIN_SEEDS[:3]):
        n, clauses = families.fan(100, seed)
        st, model, _ = exact_model.search(n, clauses, None, exact_wide.PLAIN_BUDGET)
        base = np.asarray(model, dtype=np.float32) if st == 1 else np.zeros(zc.size((n, clauses)), dtype=np.float32)
        if k < 2:
            w = base.copy()
            w[::7] = np.where(base[::7] > 0.5, np.float32(0.8), np.float32(0.3))
        else:
            w = zc.around(base, 0.9)
        inst.append((n, clauses))
        weights.append(w)
    return inst, weights


def build_batch():
    "the instances and weights of the big batch: list of (n, clauses), list of float32 arrays"
    inst, weights = [], []
    for kind in ('half', 'eighths', 'random'):
        inst += cs.family()
        weights += zc.family_weights(kind)
    rng = np.random.RandomState(60150)
    for k in cs.FAN_K:                                                                   # x1 false first: k forced variables on one level
        for lead in (0.0, 0.25):
            w = rng.uniform(0.5, 1.0, size=k + 1).astype(np.float32)
            w[0] = lead
            inst.append(cs.fan(k))
            weights.append(w)
    wi, ww = wide_cases()
    inst += wi
    weights += ww
    threesat = [pair for n in (20, 30) for pair in zc.satisfiable_3sat(100 + n, n, (3.5, 4.0, 4.5), 4)]
    for i in cs.uniform_3sat(N50_SEED, 50, (3.5, 4.0, 4.5), 3):                          # test_exact_count_gpu.py's: under 2^22 reads
        st, model, _ = exact_model.search(*i)
        threesat.append((i, np.asarray(model, dtype=np.float32) if st == 1 else np.zeros(50, dtype=np.float32)))
    for i, model in threesat:
        for w in (zc.around(model, 0.7), zc.around(model, 0.9), zc.random32(rng, i[0])):
            inst.append(i)
            weights.append(w)
    return inst, weights


@pytest.fixture(scope='module')
def batch():
    inst, weights = build_batch()
    want = zm.solve(inst, weights, BATCH_BUDGET)
    n50 = [k for k, i in enumerate(inst) if i[0] == 50]
    assert len(n50) == 27 and (want[0][n50] == 1).all() and (want[4][n50] < BATCH_BUDGET).all()      # all finish under 2^22 reads
    p = problem(inst)
    return inst, weights, want, run(inst, weights, BATCH_BUDGET, prob=p), p


def test_equal_to_the_python_model_exactly(batch):
    inst, weights, want, got, _ = batch
    assert len(inst) >= 500
    print('mass: %d instances, %d with mass, %d at the budget, leaves max %d, work max %d' %
          (len(inst), int((got[1] > 0).sum()), int((got[0] == -1).sum()), int(got[5].max()), int(got[4].max())))
    zc.same(got, want)
    assert set(np.unique(got[0])) == {-1, 1}
    assert int((got[1] > 0).sum()) >= 300 and int((got[1] == 0).sum()) >= 50 and got[5].max() > 500
    assert ((got[0] == -1) & (got[3] > 0)).any() and (got[3][got[0] == 1] == 0).all()
    few = 3 * len(cs.family())
    for j, k in enumerate((60, 60, 150, 150)):                                           # the fans: the butterfly of ascending chunks
        w = [float(x) for x in weights[few + j]]
        first = 1.0 - w[0]
        for base in range(0, k, 64):
            first = first * zm.chunk_product(w[1 + base:1 + base + 64])
        assert got[1][few + j] == first + w[0] and got[5][few + j] == (2 if w[0] else 1)


def test_half_weights_are_the_count_on_one_handle():
    inst = cs.family() + [cs.fan(k) for k in cs.FAN_K] + cs.uniform_3sat(20, 20, (3.5, 4.0, 4.5), 6)
    p = problem(inst)
    mass = run(inst, [zc.half(zc.size(i)) for i in inst], prob=p)
    st, count, tc, work, leaves = [t.cpu().numpy() for t in p.exact_count(stats=True)]
    scale = np.array([2.0 ** zc.size(i) for i in inst])
    np.testing.assert_array_equal(mass[0], st)
    np.testing.assert_array_equal(mass[1] * scale, count)
    np.testing.assert_array_equal(np.concatenate([t * s for t, s in zip(mass[2], scale)]), tc)
    np.testing.assert_array_equal(mass[4], work)
    np.testing.assert_array_equal(mass[5], leaves)
    assert not mass[3].any() and (count > 0).sum() > 200 and leaves.max() > 50


def test_eighths_equal_rational_arithmetic():
    inst, weights = zc.small()
    got = run(inst, weights)
    assert (got[0] == 1).all() and not got[3].any()
    for j, (z, true) in enumerate(zc.small_brute()):
        assert Fraction(float(got[1][j])) == z and [Fraction(float(x)) for x in got[2][j]] == true


def test_zero_one_weights_from_the_deciding_search():
    inst = [i for i, _ in zc.satisfiable_3sat(150, 50, (4.0, 4.2), 6)]
    p = problem(inst)
    st, model, _ = p.exact_solve()
    assert (st == 1).all()
    got = [t.cpu().numpy() for t in p.exact_mass(model, stats=True)]
    count = [t.cpu().numpy() for t in p.exact_count(stats=True)]
    assert (got[0] == 1).all() and (got[1] == 1.0).all() and not got[3].any() and (got[5] == 1).all()
    np.testing.assert_array_equal(got[2], model.cpu().numpy().astype(np.float64))        # the posterior is the model
    many = count[4] > 1
    assert many.sum() >= 6 and (got[4][many] < count[3][many]).all() and (got[4] <= count[3]).all()
    zc.same(run(inst, np.split(model.cpu().numpy(), len(inst)), prob=p), zm.solve(inst, np.split(model.cpu().numpy(), len(inst))))


def test_budget():
    rng = np.random.RandomState(5)
    inst = cs.family()[::5]
    weights = [zc.eighths(rng, zc.size(i)) for i in inst]
    for (i, model), conf in zip(zc.satisfiable_3sat(184, 30, (3.5, 4.0), 6), (0.5, 0.7, 0.9, 0.99) * 3):
        inst.append(i)
        weights.append(zc.around(model, conf))
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    full = run(inst, weights, prob=p)
    assert (full[0] == 1).all()
    last = None
    seen = set()
    for budget in (1, 2000, 50000):
        got = run(inst, weights, budget, prob=p)
        st, mass, tms, open_mass, work, leaves = got
        print('budget %d: complete %d of %d, mass sum %g, open sum %g' % (budget, int((st == 1).sum()), len(inst), mass.sum(), open_mass.sum()))
        zc.same(got, zm.solve(inst, weights, budget))
        assert set(np.unique(st)) <= {-1, 1}
        assert (work < budget + 3 * edges).all() and (work[st == -1] >= budget).all()
        assert last is None or (mass >= last).all()
        for j, i in enumerate(inst):
            zc.check_bracket(zc.size(i), (st[j], mass[j], None, open_mass[j]), full[1][j], full[5][j])
        last = mass
        seen |= set(np.unique(st))
    assert seen == {-1, 1} and ((st == -1) & (mass > 0) & (open_mass > 0)).any()


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_exact_mass_gpu as t
inst, weights = t.small_batch()
p = t.problem(inst)
r = t.run(inst, weights, prob=p)
np.savez(sys.argv[1], st=r[0], mass=r[1], tm=np.concatenate(r[2]), open=r[3], work=r[4], leaves=r[5], grid=p.exact_last_grid())
"""


def small_batch():
    inst = cs.family() + [cs.fan(k) for k in cs.FAN_K]
    rng = np.random.RandomState(11)
    return inst, zc.family_weights('random') + [rng.uniform(0.4, 1.0, size=k + 1).astype(np.float32) for k in cs.FAN_K]


def test_deterministic_and_instance_local(batch, tmp_path):
    from pdp import native
    inst, weights, _, a, p = batch
    zc.same(a, run(inst, weights, BATCH_BUDGET, prob=p))                                  # a second call on one handle
    order = np.random.RandomState(6).permutation(len(inst))
    zc.same(zc.pick(a, order), run([inst[i] for i in order], [weights[i] for i in order], BATCH_BUDGET))      # a shuffled batch
    for i in list(range(0, len(inst), 97)) + [len(inst) - 1]:                             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            zc.same(zc.pick(a, [i]), run([inst[i]], [weights[i]], BATCH_BUDGET))
    prev = native.use_build('fast')
    try:
        fast = run(inst, weights, BATCH_BUDGET)
    finally:
        native.use_build(prev)
    zc.same(a, fast)
    # one wave takes every instance, one after the other, in a process of its own
    sinst, sweights = small_batch()
    here = run(sinst, sweights)
    out = str(tmp_path / 'one.npz')
    env = dict(os.environ, PDP_EXACT_GRID='1')
    r = subprocess.run([sys.executable, '-c', CHILD % (os.path.join(REPO, 'tests'), os.path.join(REPO, 'pdp-solver_amd')), out], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    one = np.load(out)
    assert int(one['grid']) == 1
    for k, name in ((0, 'st'), (1, 'mass'), (3, 'open'), (4, 'work'), (5, 'leaves')):
        np.testing.assert_array_equal(here[k], one[name])
    np.testing.assert_array_equal(np.concatenate(here[2]), one['tm'])


def test_hbm_route():
    "an instance past the slab inside a batch of small ones: equal to rational arithmetic and to the model, and the same alone"
    big = cs.past_the_slab()
    rng = np.random.RandomState(92)
    wbig = zc.eighths(rng, 10)
    wbig[wbig == 0] = 0.125                                                               # keep the whole tree
    few, wfew = zc.small()[0][:40], zc.small()[1][:40]
    inst, weights = few[:20] + [big] + few[20:], wfew[:20] + [wbig] + wfew[20:]
    got = run(inst, weights)
    want = zm.search(*big, wbig)
    assert (got[0][20], got[1][20], got[3][20], got[4][20], got[5][20]) == (want[0], want[1], want[3], want[4], want[5])
    assert np.array_equal(got[2][20], want[2]) and want[5] >= 5
    z, true = zc.brute(*big, wbig)
    assert Fraction(float(got[1][20])) == z and [Fraction(float(x)) for x in got[2][20]] == true
    rest = [i for i in range(len(inst)) if i != 20]
    for i, (z, true) in zip(rest, zc.small_brute()[:40]):
        assert Fraction(float(got[1][i])) == z and [Fraction(float(x)) for x in got[2][i]] == true
    zc.same(zc.pick(got, [20]), run([big], [wbig]))


def test_refused_instances_among_small_ones():
    few, wfew = zc.small()[0][:6], zc.small()[1][:6]
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    soft = (12, [[1, 2], [-1, 12], [3, -5, 7]])
    nan_w, big_w = np.full(12, 0.25, dtype=np.float32), np.full(12, 0.75, dtype=np.float32)
    nan_w[70 % 12], big_w[11] = np.nan, 1.5
    inst = few[:2] + [wide] + few[2:4] + [soft] + few[4:] + [soft]
    weights = wfew[:2] + [zc.half(1024)] + wfew[2:4] + [nan_w] + wfew[4:] + [big_w]
    got = run(inst, weights)
    assert got[0].tolist() == [1, 1, -2, 1, 1, -3, 1, 1, -3]
    for j in (2, 5, 8):
        assert (got[1][j], got[3][j], got[4][j], got[5][j]) == (0.0, 0.0, 0, 0) and got[2][j].shape == (zc.size(inst[j]),) and not got[2][j].any()
    rest = [i for i in range(len(inst)) if i not in (2, 5, 8)]
    zc.same(zc.pick(got, rest), zm.solve([inst[i] for i in rest], [weights[i] for i in rest]))
    for i in rest:                                                                        # every neighbour equals its value alone
        if sum(len(c) for c in inst[i][1]) > 0:
            zc.same(zc.pick(got, [i]), run([inst[i]], [weights[i]]))
    zc.same(zc.pick(got, [2, 5, 8]), zm.solve([inst[i] for i in (2, 5, 8)], [weights[i] for i in (2, 5, 8)]))


def test_one_handle_interleaved():
    inst, weights = small_batch()
    p = problem(inst)
    w = device_weights(weights)
    pull = lambda r: [t.cpu().numpy() for t in r]                                         # noqa: E731
    c0, m0, s0 = pull(p.exact_count(stats=True)), pull(p.exact_mass(w, stats=True)), pull(p.exact_solve())
    m1, c1 = pull(p.exact_mass(w, stats=True)), pull(p.exact_count(stats=True))
    for a, b in ((c0, c1), (m0, m1)):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    zc.same(run(inst, weights, prob=p), zm.solve(inst, weights))
    assert (s0[0][m0[1] > 0] == 1).all()                                                  # mass only where there is a model


def test_refusals():
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(4, 20, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    w = torch.full((p.V,), 0.5, dtype=torch.float32, device=p.device)
    outs = [torch.full((p.B,), 7, dtype=torch.int8, device=p.device), torch.full((p.B,), 7.0, dtype=torch.float64, device=p.device),
            torch.full((p.V,), 7.0, dtype=torch.float64, device=p.device), torch.full((p.B,), 7.0, dtype=torch.float64, device=p.device)]
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_mass(w)
    assert native.lib().pdp_exact_mass(p._h, native.ptr(w), ctypes.c_int64(0), *[native.ptr(t) for t in outs], None, None, None) == 4
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)                                        # no output was touched
    p = native.Problem(*args)
    w = torch.full((p.V,), 0.5, dtype=torch.float32, device=p.device)
    for wrong in (w.cpu(), w.double(), w[:-1], torch.cat([w, w])[::2], None, w.tolist()):
        with pytest.raises(native.NativeError):
            p.exact_mass(wrong)
    assert p.exact_last_grid() == 0                                                       # nothing was launched
    for wrong in (1.5, '7', None, True):
        with pytest.raises(ValueError):
            p.exact_mass(w, budget=wrong)
    st, mass, tm, open_mass, work = p.exact_mass(w)
    assert (st.dtype, mass.dtype, tm.dtype, open_mass.dtype, work.dtype) == (torch.int8, torch.float64, torch.float64, torch.float64, torch.int64)
    assert (mass.numel(), tm.numel(), open_mass.numel()) == (p.B, p.V, p.B)
    outs = [st, mass, tm, open_mass]
    null = [(None, outs[0], outs[1], outs[2], outs[3]), (w, None, outs[1], outs[2], outs[3]), (w, outs[0], None, outs[2], outs[3]),
            (w, outs[0], outs[1], None, outs[3]), (w, outs[0], outs[1], outs[2], None)]
    for a in null:                                                                        # NULL weights or outputs
        assert native.lib().pdp_exact_mass(p._h, native.ptr(a[0]), ctypes.c_int64(0), *[native.ptr(t) for t in a[1:]], None, None, None) != native.PDP_OK


def test_solution_mass_segments_and_items_without_a_literal():
    from pdp import exact
    items = [exact.raw_item(3, []), exact.raw_item(2, [[], []]), exact.raw_item(4, [[]]), exact.raw_item(1024, []), exact.raw_item(2, [])]
    weights = [[0.25, 0.5, 1.0], [0.5, 0.5], [0.5] * 4, [0.5] * 1024, [0.5, np.nan]]
    st, mass, post, open_mass, work = exact.solution_mass(items, weights)
    assert st.tolist() == [1, 1, 1, -2, -3] and mass.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and not open_mass.any() and not work.any()
    assert post[0].tolist() == [0.25, 0.5, 1.0] and post[0].dtype == np.float64 and all(x is None for x in post[1:])
    # through the cut along max_edges: the same answers as one problem, and rational arithmetic's
    inst, w = zc.small()[0][:60], zc.small()[1][:60]
    raw = [exact.raw_item(n, c) for n, c in inst]
    whole, cut = exact.solution_mass(raw, w), exact.solution_mass(raw, w, max_edges=100)
    assert whole[0].dtype == np.int8 and whole[1].dtype == whole[3].dtype == np.float64 and whole[4].dtype == np.int64
    for k in (0, 1, 3, 4):
        np.testing.assert_array_equal(whole[k], cut[k])
    for a, b, (z, true), ma in zip(whole[2], cut[2], zc.small_brute()[:60], whole[1]):
        assert Fraction(float(ma)) == z and (a is None) == (b is None) == (z == 0)
        if z:
            assert a.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(a, np.array([float(t) for t in true]) / ma)
    with pytest.raises(ValueError):
        exact.solution_mass(raw, w[:-1])


def test_cli_complete_mass(tmp_path):
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    from test_sharded_gpu import _run
    r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d', '--complete-mass',
                        '-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                       cwd=REPO)
    assert r.returncode != 0 and '--complete-mass' in r.stderr and 'give --complete as well' in r.stderr
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    for i in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 128)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '--complete']
    new = ['solution_mass', 'solution_mass_log2', 'solution_mass_open', 'solution_mass_proved', 'posterior', 'mass_work']
    base, _ = _run(argv + ['-w', '0'], 1, str(tmp_path / 'base.jsonl'), 0)
    soft, log = _run(argv + ['-w', '0', '--complete-mass', '-v'], 1, str(tmp_path / 'soft.jsonl'), 0)
    hard, _ = _run(argv + ['-w', '100', '--complete-mass'], 1, str(tmp_path / 'hard.jsonl'), 0)
    assert len(base) == len(soft) == len(hard) == 40
    asked = proved = fractional = 0
    for b, g in zip(base, soft):
        assert not set(new) & set(json.loads(b))                                          # without the flag: today's rows
        r = json.loads(g)
        if r['complete'] != 1:
            assert g == b                                                                # byte-identical to the run without the flag
            continue
        keys = [k for k in new if k != 'posterior' or r['solution_mass'] > 0]
        assert list(r)[-len(keys):] == keys and {k: v for k, v in r.items() if k not in new} == json.loads(b)
        mass, open_mass = r['solution_mass'], r['solution_mass_open']
        assert 0.0 <= mass <= 1.0 and 0.0 <= open_mass <= 1.0 and r['mass_work'] > 0
        assert r['solution_mass_proved'] in (0, 1) and (r['solution_mass_proved'] == 0 or open_mass == 0.0)
        assert r['solution_mass_log2'] == (float(np.log2(mass)) if mass > 0 else None)
        if mass > 0:
            post = np.asarray(r['posterior'])
            assert post.shape == (30,) and (post >= 0).all() and (post <= 1).all()
        asked += 1
        proved += r['solution_mass_proved']
        fractional += 0.0 < mass < 1.0
    print('soft run: %d rows asked, %d proved, %d with a mass strictly between 0 and 1' % (asked, proved, fractional))
    assert asked >= 5
    said = log[log.index('complete search:'):].split('\n')[0]
    assert said.endswith('; solution mass for %d of %d' % (proved, asked))
    seen = 0
    for g in hard:                                                                        # after Walk-SAT the prediction is 0/1
        r = json.loads(g)
        if r['complete'] == 1:
            assert r['solution_mass'] in (0.0, 1.0) and r['solution_mass'] == r['pdp_solved'] and r['solution_mass_proved'] == 1
            assert r['solution_mass_open'] == 0.0
            seen += 1
        else:
            assert not set(new) & set(r)
    assert seen >= 5
