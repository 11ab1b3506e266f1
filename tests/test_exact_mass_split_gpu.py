"""The split weighted counting search on the GPU (pdp_exact_mass_split, Problem.exact_mass_split, exact.solution_mass(split=), satyr.py
--complete --complete-mass --complete-mass-split): equal to its Python statement (tests/exact_mass_split_model.py) bit for bit in status,
mass, true_mass, open_mass, work, leaves, depth_used and every cube record; depth 0 equal to exact_mass; weights 0.5 equal to
exact_count_split record for record; mass, true_mass and leaves against exact_mass at n = 50 within the derived bounds; the budget per
cube; determinism of every output and record over call, batch, grid and build; the HBM route and refused instances; refusals; a count
split and a mass split interleaved on one handle; the host entry points; the command line."""
import ctypes
import faulthandler
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
import exact_mass_split_model as zs
from helpers import REPO

pytestmark = pytest.mark.gpu

SATYR = os.path.join(REPO, 'pdp-solver_amd', 'satyr.py')
PDP_YAML = os.path.join(REPO, 'config', 'Predict', 'PDP-p-d-p-sp-pytorch.yaml')
KEYS = ('status', 'mass', 'true_mass', 'open_mass', 'work', 'leaves', 'depth_used', 'cube_off', 'cube_status', 'cube_mass', 'cube_open',
        'cube_work', 'cube_leaves')
CUBE_KEYS = KEYS[8:]
STEP_LIMIT = 240        # seconds per test: a cube kernel that does not end is a hang, and ends the run with every thread's traceback


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def problem(inst):
    from pdp import exact, native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment([exact.raw_item(n, c) for n, c in inst]), torch.device('cuda:0'))
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(inst))


def widen(inst):
    return [(zc.size(i), i[1]) for i in inst]


def device_weights(weights):
    return torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.float32) for w in weights])).to('cuda:0')


def run(inst, weights, depth, budget=0, prob=None):
    "Problem.exact_mass_split(stats=True) as a dict of numpy arrays, true_mass cut per instance"
    p = problem(inst) if prob is None else prob
    d = depth if isinstance(depth, int) else torch.from_numpy(np.asarray(depth, dtype=np.int8)).cuda()
    got = dict(zip(KEYS, [t.cpu().numpy() for t in p.exact_mass_split(device_weights(weights), budget, depth=d, stats=True)]))
    assert [got[k].dtype for k in KEYS] == [np.int8, np.float64, np.float64, np.float64, np.int64, np.int64, np.int8, np.int64, np.int8,
                                            np.float64, np.float64, np.int64, np.int64]
    assert got['cube_off'][0] == 0 and np.array_equal(np.diff(got['cube_off']), 1 << got['depth_used'].astype(np.int64))
    assert all(got[k].shape == (got['cube_off'][-1],) for k in CUBE_KEYS)
    got['true_mass'] = np.split(got['true_mass'], np.cumsum([n for n, _ in inst])[:-1])
    return got


def reference(inst, weights, depth, budget=0):
    depth = [depth] * len(inst) if isinstance(depth, int) else depth
    return [zs.search(n, c, w, budget, int(d)) for (n, c), w, d in zip(inst, weights, depth)]


def same_as_model(got, want):
    "every output and every cube record against tests/exact_mass_split_model.py, bit for bit"
    for j, (st, mass, tm, open_mass, work, leaves, used, cubes) in enumerate(want):
        assert (got['status'][j], got['mass'][j], got['open_mass'][j], got['work'][j], got['leaves'][j], got['depth_used'][j]) == \
            (st, mass, open_mass, work, leaves, used), j
        assert np.array_equal(got['true_mass'][j], tm), j
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        rec = list(zip(*[got[k][a:z].tolist() for k in CUBE_KEYS]))
        assert rec == [tuple(c) for c in cubes], j


def everything(got, order=None):
    "every output and record per instance in a comparable form"
    idx = range(len(got['status'])) if order is None else order
    out = []
    for j in idx:
        a, z = got['cube_off'][j], got['cube_off'][j + 1]
        out.append((int(got['status'][j]), got['mass'][j].tobytes(), got['true_mass'][j].tobytes(), got['open_mass'][j].tobytes(),
                    int(got['work'][j]), int(got['leaves'][j]), int(got['depth_used'][j])) + tuple(got[k][a:z].tobytes() for k in CUBE_KEYS))
    return out


def build_batch():
    """about 450 instances for one problem: the host family (n <= 12), a quarter each with eighths / random float32 / 0-1 / 0.5 weights, the
    k = 150 fan at depth 2 (150 forced variables on one level: three chunks of lanes), uniform 3-SAT of n = 20 / 30 at clause ratios 3.5,
    4.0 and 4.5 with soft weights; depths mixed over 0..6"""
    few = cs.family()
    rng = np.random.RandomState(914)
    kinds = (zc.family_weights('eighths'), zc.family_weights('random'), None, zc.family_weights('half'))
    weights = []
    for j, i in enumerate(few):
        w = kinds[j % 4]
        weights.append((rng.rand(zc.size(i)) < 0.5).astype(np.float32) if w is None else w[j])
    inst = list(few)
    for lead in (0.0, 0.25):                                                              # x1 false first where it is the heavier literal
        w = rng.uniform(0.5, 1.0, size=151).astype(np.float32)
        w[0] = lead
        inst.append(cs.fan(150))
        weights.append(w)
    for n in (20, 30):
        for i in cs.uniform_3sat(n, n, (3.5, 4.0, 4.5), 3):
            inst += [i, i]
            weights += [rng.uniform(0.05, 0.95, size=n).astype(np.float32), zc.random32(rng, n)]
    depth = np.random.RandomState(7).randint(0, 7, size=len(inst)).astype(np.int8)
    depth[len(few):len(few) + 2] = 2
    return widen(inst), weights, depth


@pytest.fixture(scope='module')
def batch():
    "the batch, the model's answers computed once, and one handle"
    inst, weights, depth = build_batch()
    return inst, weights, depth, reference(inst, weights, depth), problem(inst)


def test_equal_to_the_python_model_exactly(batch):
    inst, weights, depth, want, p = batch
    assert len(inst) >= 440 and set(depth.tolist()) == set(range(7))
    got = run(inst, weights, depth, prob=p)
    inside = sum(1 for w in want if len(w[7]) > 1 and any(c[4] == 0 and c[3] > 0 for c in w[7]))
    print('mass split: %d instances, %d cubes, %d with mass, %d cubes without mass, leaves max %d'
          % (len(inst), len(got['cube_status']), int((got['mass'] > 0).sum()), int((got['cube_mass'] == 0).sum()), int(got['leaves'].max())))
    same_as_model(got, want)
    assert (got['status'] == 1).all() and not got['open_mass'].any() and not got['cube_open'].any()
    assert int((got['mass'] > 0).sum()) > 200 and int((got['mass'] == 0).sum()) > 50 and inside > 100
    few = cs.family()
    for j, (i, w) in enumerate(zip(few, weights)):                                        # rational arithmetic where every operation is exact
        if j % 4 in (0, 2, 3):
            z, true = zc.brute(zc.size(i), i[1], w)
            assert Fraction(float(got['mass'][j])) == z and [Fraction(float(x)) for x in got['true_mass'][j]] == true, j
    for j in (len(few), len(few) + 1):
        assert got['depth_used'][j] == 2 and got['leaves'][j] >= 1 and got['mass'][j] > 0


def test_depth_zero_is_exact_mass(batch):
    inst, weights, _, _, p = batch
    plain = [t.cpu().numpy() for t in p.exact_mass(device_weights(weights), stats=True)]
    zero = run(inst, weights, 0, prob=p)
    for k, want in zip(KEYS[:6], plain):
        got = np.concatenate(zero[k]) if k == 'true_mass' else zero[k]
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    assert not zero['depth_used'].any() and np.array_equal(zero['cube_off'], np.arange(len(inst) + 1))
    assert np.array_equal(zero['cube_status'], plain[0]) and np.array_equal(zero['cube_mass'], plain[1])
    assert np.array_equal(zero['cube_open'], plain[3]) and np.array_equal(zero['cube_work'], plain[4])
    assert np.array_equal(zero['cube_leaves'], plain[5])


def test_half_weights_are_exact_count_split_record_for_record(batch):
    inst, _, depth, _, p = batch
    half = [zc.half(n) for n, _ in inst]
    d = torch.from_numpy(depth).cuda()
    for budget in (0, 3000):
        got = run(inst, half, depth, budget, prob=p)
        cnt = [t.cpu().numpy() for t in p.exact_count_split(budget, depth=d, stats=True)]
        scale = np.array([2.0 ** n for n, _ in inst])
        assert np.array_equal(got['status'], cnt[0]) and np.array_equal(got['work'], cnt[3]) and np.array_equal(got['leaves'], cnt[4])
        assert np.array_equal(got['depth_used'], cnt[5]) and np.array_equal(got['cube_off'], cnt[6])
        assert np.array_equal(got['cube_status'], cnt[7]) and np.array_equal(got['cube_work'], cnt[9])
        assert np.array_equal(got['cube_leaves'], cnt[10])
        per_cube = np.repeat(scale, 1 << depth.astype(np.int64))
        assert np.array_equal(got['cube_mass'] * per_cube, cnt[8])
        sure = cnt[1] <= 2.0 ** 53                                                        # above, the count rounds where the mass does not
        assert np.array_equal((got['mass'] * scale)[sure], cnt[1][sure]) and sure.sum() >= len(inst) - 2
        tc = np.split(cnt[2], np.cumsum([n for n, _ in inst])[:-1])
        assert all(np.array_equal(got['true_mass'][j] * scale[j], tc[j]) for j in np.nonzero(sure)[0])
    assert (got['status'] == -1).any() and (got['status'] == 1).any()


def test_equal_to_exact_mass_at_n_50():
    inst = cs.uniform_3sat(57, 50, (4.0, 4.26, 4.5, 5.0), 8)
    rng = np.random.RandomState(50)
    weights = [rng.uniform(0.1, 0.9, size=50).astype(np.float32) for _ in inst]
    model = zm.solve(inst, weights, 1 << 22)
    assert len(inst) == 32 and (model[0] == 1).all() and (model[4] < 1 << 22).all()      # all finish under 2^22 reads
    p = problem(inst)
    st, mass, tm, open_mass, work, leaves = [t.cpu().numpy() for t in p.exact_mass(device_weights(weights), stats=True)]
    zc.same((st, mass, np.split(tm, 32), open_mass, work, leaves), model)
    assert (mass > 0).sum() >= 8
    for depth in (6, 10):
        got = run(inst, weights, depth, prob=p)
        print('n=50 depth %d: work ratio to the plain mass %.2f, cubes without mass %d of %d, worst |mass - plain| / bound %.3f'
              % (depth, got['work'].sum() / work.sum(), int((got['cube_mass'] == 0).sum()), len(got['cube_mass']),
                 max(abs(got['mass'][j] - mass[j]) / (zm.mass_bound(50, 2 * leaves[j] + (1 << depth), mass[j]) or 1.0) for j in range(32))))
        assert (got['depth_used'] == depth).all() and np.array_equal(got['status'], st) and not got['open_mass'].any()
        assert np.array_equal(got['leaves'], leaves) and (got['work'] >= work).all()
        for j in range(32):
            # both sides within their own bound of the exact value: the plain search's, and the split sum's with one more rounding per
            # cube (exact_mass_model's bounds with leaves + cubes); the mass itself stands in for Z*, within 1 + 1e-9
            z = mass[j] * (1 + 1e-9)
            k = int(leaves[j]) + (1 << depth)
            assert abs(got['mass'][j] - mass[j]) <= zm.mass_bound(50, leaves[j], z) + zm.mass_bound(50, k, z), j
            limit = zm.true_mass_bound(50, leaves[j], z) + zm.true_mass_bound(50, k, z)
            assert (np.abs(got['true_mass'][j] - tm[50 * j:50 * j + 50]) <= limit).all(), j
            assert (got['mass'][j] == 0.0) == (mass[j] == 0.0)
        assert p.exact_last_grid() > 32                     # more waves at work than instances


def test_budget_per_cube():
    rng = np.random.RandomState(5)
    inst = cs.family()[::5]
    weights = [zc.eighths(rng, zc.size(i)) for i in inst]
    for (i, model), conf in zip(zc.satisfiable_3sat(184, 30, (3.5, 4.0), 6), (0.5, 0.7, 0.9, 0.99) * 3):
        inst.append(i)
        weights.append(zc.around(model, conf))
    inst = widen(inst)
    depth = np.random.RandomState(8).randint(0, 5, size=len(inst)).astype(np.int8)
    edges = np.array([sum(len(c) for c in cl) for _, cl in inst])
    p = problem(inst)
    full = run(inst, weights, depth, prob=p)
    assert (full['status'] == 1).all()
    seen = set()
    for budget in (2000, 50000):
        got = run(inst, weights, depth, budget, prob=p)
        same_as_model(got, reference(inst, weights, depth, budget))
        per_cube = np.repeat(edges, 1 << depth.astype(np.int64))
        assert (got['cube_work'] < budget + 3 * per_cube).all() and (got['cube_work'][got['cube_status'] == -1] >= budget).all()
        assert (got['work'] < (1 << depth.astype(np.int64)) * (budget + 3 * edges)).all() and (got['leaves'] <= full['leaves']).all()
        assert not got['cube_open'][got['cube_status'] == 1].any()
        for j, (n, _) in enumerate(inst):
            a, z = got['cube_off'][j], got['cube_off'][j + 1]
            assert got['status'][j] == (-1 if (got['cube_status'][a:z] == -1).any() else 1)
            k = int(full['leaves'][j]) + int(z - a)
            slack = zm.mass_bound(n, k, 1.0)
            assert got['mass'][j] <= full['mass'][j] * (1 + slack)
            assert full['mass'][j] <= (got['mass'][j] + got['open_mass'][j]) * (1 + slack)
            assert got['mass'][j] + got['open_mass'][j] <= 1 + slack
        seen |= set(got['status'].tolist())
    assert seen == {-1, 1} and ((got['status'] == -1) & (got['mass'] > 0) & (got['open_mass'] > 0)).any()


def small_batch():
    "what the child process of the grid test runs: every fourth instance of the batch"
    inst, weights, depth = build_batch()
    return inst[::4], weights[::4], depth[::4]


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_exact_mass_split_gpu as t
inst, weights, depth = t.small_batch()
p = t.problem(inst)
r = t.run(inst, weights, depth, prob=p)
r['true_mass'] = np.concatenate(r['true_mass'])
np.savez(sys.argv[1], grid=p.exact_last_grid(), **r)
"""


def test_deterministic_in_every_output_and_record(batch, tmp_path):
    from pdp import native
    inst, weights, depth, _, p = batch
    got = run(inst, weights, depth, prob=p)
    a = everything(got)
    assert a == everything(run(inst, weights, depth, prob=p))                             # a second call on one handle
    assert p.exact_last_grid() > 1
    order = np.random.RandomState(6).permutation(len(inst))
    assert [a[i] for i in order] == everything(run([inst[i] for i in order], [weights[i] for i in order], depth[order]))      # a shuffled batch
    for i in list(range(0, len(inst), 61)) + [len(inst) - 1]:                             # alone
        if sum(len(c) for c in inst[i][1]) > 0:
            assert [a[i]] == everything(run([inst[i]], [weights[i]], depth[i:i + 1]))
    prev = native.use_build('fast')
    try:
        fast = run(inst, weights, depth)
    finally:
        native.use_build(prev)
    assert a == everything(fast)
    # one wave takes every cube, one after the other, in a process of its own
    out = str(tmp_path / 'one.npz')
    env = dict(os.environ, PDP_EXACT_GRID='1')
    r = subprocess.run([sys.executable, '-c', CHILD % (os.path.join(REPO, 'tests'), os.path.join(REPO, 'pdp-solver_amd')), out], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=STEP_LIMIT, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    one = dict(np.load(out))
    assert int(one.pop('grid')) == 1
    sinst = small_batch()[0]
    one['true_mass'] = np.split(one['true_mass'], np.cumsum([n for n, _ in sinst])[:-1])
    assert everything(one) == a[::4]


def test_hbm_route_is_weighed_at_depth_zero():
    big = cs.past_the_slab()
    rng = np.random.RandomState(92)
    wbig = zc.eighths(rng, 10)
    wbig[wbig == 0] = 0.125                                                               # keep the whole tree
    few, wfew = zc.small()[0][:40], zc.small()[1][:40]
    inst, weights = widen(few[:20] + [big] + few[20:]), wfew[:20] + [wbig] + wfew[20:]
    p = problem(inst)
    got = run(inst, weights, 3, prob=p)
    want = zm.search(*big, wbig)
    assert got['depth_used'][20] == 0 and (np.delete(got['depth_used'], 20) == 3).all()
    assert (got['status'][20], got['mass'][20], got['open_mass'][20], got['work'][20], got['leaves'][20]) == \
        (want[0], want[1], want[3], want[4], want[5])
    assert np.array_equal(got['true_mass'][20], want[2])
    a = int(got['cube_off'][20])
    assert got['cube_off'][21] == a + 1
    assert tuple(got[k][a] for k in CUBE_KEYS) == (want[0], want[1], want[3], want[4], want[5])
    rest = [i for i in range(len(inst)) if i != 20]
    for i, (z, true) in zip(rest, zc.small_brute()[:40]):
        assert Fraction(float(got['mass'][i])) == z and [Fraction(float(x)) for x in got['true_mass'][i]] == true
    alone = run([inst[20]], [wbig], 3)
    assert alone['depth_used'].tolist() == [0] and everything(alone) == everything(got, [20])


def test_refused_instances_among_small_ones():
    few, wfew = widen(zc.small()[0][:6]), zc.small()[1][:6]
    wide = (1024, [[1, 2], [-1, 1024], [3, -500, 700]])
    soft = (12, [[1, 2], [-1, 12], [3, -5, 7]])
    nan_w, big_w = np.full(12, 0.25, dtype=np.float32), np.full(12, 0.75, dtype=np.float32)
    nan_w[70 % 12], big_w[11] = np.nan, 1.5
    inst = few[:2] + [wide] + few[2:4] + [soft] + few[4:] + [soft]
    weights = wfew[:2] + [zc.half(1024)] + wfew[2:4] + [nan_w] + wfew[4:] + [big_w]
    depth = [2, 0, 4, 5, 1, 3, 6, 2, 0]
    got = run(inst, weights, depth)
    assert got['status'].tolist() == [1, 1, -2, 1, 1, -3, 1, 1, -3] and got['depth_used'].tolist() == [2, 0, 0, 5, 1, 3, 6, 2, 0]
    for j in (2, 5, 8):
        assert (got['mass'][j], got['open_mass'][j], got['work'][j], got['leaves'][j]) == (0.0, 0.0, 0, 0)
        assert got['true_mass'][j].shape == (inst[j][0],) and not got['true_mass'][j].any()
    a, z = got['cube_off'][5], got['cube_off'][6]
    assert z - a == 8 and (got['cube_status'][a:z] == -3).all() and not got['cube_mass'][a:z].any() and not got['cube_work'][a:z].any()
    same_as_model(got, reference(inst, weights, depth))
    for j, d in ((2, 7), (5, 3), (8, 0)):                                                 # and alone
        assert everything(run([inst[j]], [weights[j]], d)) == everything(got, [j])


def test_refusals(tmp_path):
    from pdp import native
    from pdp.factorgraph import dataset
    native.require_gpu()
    b = dataset.to_torch(dataset.collate_segment(dataset.random_ksat_items(80, 8, 3, seed=1)), torch.device('cuda:0'))
    args = (b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'])
    p = native.Problem(*args, replication=2)
    with pytest.raises(native.NativeError, match='error 4'):
        p.exact_mass_split(torch.full((p.V,), 0.5, dtype=torch.float32, device=p.device), depth=2)
    p = native.Problem(*args)
    w = torch.full((p.V,), 0.5, dtype=torch.float32, device=p.device)
    cubes = (torch.empty(p.B + 1, dtype=torch.int64, device=p.device), torch.empty(1 << 10, dtype=torch.int8, device=p.device),
             torch.empty(1 << 10, dtype=torch.float64, device=p.device), torch.empty(1 << 10, dtype=torch.float64, device=p.device),
             torch.empty(1 << 10, dtype=torch.int64, device=p.device), torch.empty(1 << 10, dtype=torch.int64, device=p.device))
    assert native.lib().pdp_exact_mass_split_cubes(p._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK        # no split call yet
    for wrong, at in ((17, 5), (-1, 63)):
        depth = torch.zeros(p.B, dtype=torch.int8, device=p.device)
        depth[at] = wrong
        depth[70] = wrong
        with pytest.raises(native.NativeError, match='pdp_exact_mass_split: the depth of instance %d is not in 0 .. 16' % at):
            p.exact_mass_split(w, 1, depth=depth)
    # every call that must be refused runs with a budget of one read: should a refusal ever fail, its cubes end after one pass each
    with pytest.raises(native.NativeError, match=r'more than 2\^22 cubes in one call \(reached at instance 64\)'):
        p.exact_mass_split(w, 1, depth=16)                                                  # 80 * 2^16
    # the rows: cubes x n_max x 8 bytes.  At n = 8 the cube cap comes first; 12 instances of 600 variables (most of them in no clause:
    # raw_item keeps them) pass 2^31 bytes at the seventh: 7 * 2^16 * 600 * 8 > 2^31 >= 6 * 2^16 * 600 * 8
    rng = np.random.RandomState(2)
    q = problem([(600, [[int(v) * int(s) for v, s in zip(rng.choice(600, size=3, replace=False) + 1, rng.choice([-1, 1], size=3))]
                        for _ in range(60)]) for _ in range(12)])
    assert q.V == 12 * 600
    wq = torch.full((q.V,), 0.5, dtype=torch.float32, device=q.device)
    with pytest.raises(native.NativeError, match=r'per-cube rows \(cubes x 600 variables x 8 bytes\) pass 2\^31 bytes at instance 6'):
        q.exact_mass_split(wq, 1, depth=16)
    assert native.lib().pdp_exact_mass_split_cubes(q._h, *[native.ptr(t) for t in cubes], None) != native.PDP_OK        # a refused call leaves none
    ok = torch.zeros(q.B, dtype=torch.int8, device=q.device)
    ok[:6] = 12
    st, mass, _, open_mass = q.exact_mass_split(wq, 1, depth=ok)[:4]                        # 6 * 2^12 + 6 cubes of 600 variables: allowed
    assert (st.cpu().numpy() == -1).all() and not mass.cpu().numpy().any()                  # one read each: nothing is weighed
    np.testing.assert_array_equal(open_mass.cpu().numpy(), np.ones(q.B))                    # 0.5 + 0.5 from the two cubes that own a node
    for wrong in (1.5, '7', True, torch.zeros(p.B), torch.zeros(p.B - 1, dtype=torch.int8, device=p.device), torch.zeros(p.B, dtype=torch.int8)):
        with pytest.raises(ValueError):
            p.exact_mass_split(w, depth=wrong)
    for wrong in (1.5, '7', None, True):
        with pytest.raises(ValueError):
            p.exact_mass_split(w, budget=wrong)
    for wrong in (w.cpu(), w.double(), w[:-1], None, w.tolist()):
        with pytest.raises(native.NativeError):
            p.exact_mass_split(wrong, depth=1)
    status = torch.empty(p.B, dtype=torch.int8, device=p.device)
    assert native.lib().pdp_exact_mass_split(p._h, native.ptr(w), None, ctypes.c_int64(0), native.ptr(status), None, None, None, None, None, None,
                                             None) != native.PDP_OK
    st = p.exact_mass_split(w, depth=3)[0]
    assert (st.cpu().numpy() == 1).all()
    for argv, said in ((['--complete', '--complete-mass-split', '3'], 'give --complete-mass as well'),
                       (['--complete', '--complete-mass', '--complete-mass-split', '17'], 'takes a depth from 0 to 16'),
                       (['--complete', '--complete-mass', '--complete-mass-split', '-2'], 'takes a depth from 0 to 16')):
        r = subprocess.run([sys.executable, SATYR, PDP_YAML, os.path.join(REPO, 'tests', 'golden', 'dimacs20'), '10', '-d'] + argv +
                           ['-o', str(tmp_path / 'no.jsonl')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300,
                           cwd=REPO)
        assert r.returncode != 0 and '--complete-mass-split' in r.stderr and said in r.stderr


def test_count_split_and_mass_split_interleaved_on_one_handle(batch):
    from pdp import native
    inst, weights, depth, _, p = batch
    w = device_weights(weights)
    dm = torch.from_numpy(depth).cuda()
    dc = torch.from_numpy(((depth.astype(np.int64) + 3) % 7).astype(np.int8)).cuda()          # other depths: other cube counts
    pull = lambda r: [t.cpu().numpy() for t in r]                                         # noqa: E731

    def mass_cubes(total):
        out = (torch.empty(p.B + 1, dtype=torch.int64, device=p.device), torch.empty(total, dtype=torch.int8, device=p.device),
               torch.empty(total, dtype=torch.float64, device=p.device), torch.empty(total, dtype=torch.float64, device=p.device),
               torch.empty(total, dtype=torch.int64, device=p.device), torch.empty(total, dtype=torch.int64, device=p.device))
        assert native.lib().pdp_exact_mass_split_cubes(p._h, *[native.ptr(t) for t in out], None) == native.PDP_OK
        return pull(out)

    def count_cubes(total):
        out = (torch.empty(p.B + 1, dtype=torch.int64, device=p.device), torch.empty(total, dtype=torch.int8, device=p.device),
               torch.empty(total, dtype=torch.float64, device=p.device), torch.empty(total, dtype=torch.int64, device=p.device),
               torch.empty(total, dtype=torch.int64, device=p.device))
        assert native.lib().pdp_exact_count_split_cubes(p._h, *[native.ptr(t) for t in out], None) == native.PDP_OK
        return pull(out)

    m0 = pull(p.exact_mass_split(w, depth=dm, stats=True))
    c0 = pull(p.exact_count_split(depth=dc, stats=True))
    kept = mass_cubes(len(m0[8]))                                                           # the mass records behind a count call
    for x, y in zip(kept, m0[7:]):
        np.testing.assert_array_equal(x, y)
    m1 = pull(p.exact_mass_split(w, depth=dm, stats=True))
    kept = count_cubes(len(c0[7]))                                                          # the count records behind a mass call
    for x, y in zip(kept, c0[6:]):
        np.testing.assert_array_equal(x, y)
    c1 = pull(p.exact_count_split(depth=dc, stats=True))
    for a, b in ((m0, m1), (c0, c1)):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    assert len(m0[8]) != len(c0[7])


def test_solution_mass_split_on_segments_and_items_without_a_literal(monkeypatch):
    from pdp import exact
    inst = cs.family()[:120] + cs.uniform_3sat(150, 30, (3.5, 4.26, 5.0), 3)
    rng = np.random.RandomState(44)
    w = zc.family_weights('eighths')[:120] + [(rng.randint(1, 8, size=30) / 8.0).astype(np.float32) for _ in range(9)]
    raw = [exact.raw_item(3, []), exact.raw_item(2, [[], []])] + [exact.raw_item(n, c) for n, c in inst] + \
        [exact.raw_item(4, [[]]), exact.raw_item(1024, []), exact.raw_item(1024, [[1, 2], [-1, 1024]]), exact.raw_item(2, [[1, 2]])]
    weights = [[0.25, 0.5, 1.0], [0.5, 0.5]] + w + [[0.5] * 4, [0.5] * 1024, [0.5] * 1024, [0.5, np.nan]]
    base = exact.solution_mass(raw, weights)
    assert set(base[0].tolist()) == {-3, -2, 1} and base[0][-1] == -3 and not base[3].any()
    monkeypatch.setattr(exact, 'AUTO_MASS_STAGE1_BUDGET', 300)                            # so that the second stage has work to do
    for split in (4, 'auto'):
        for max_edges in (exact.MAX_EDGES, 400):
            got = exact.solution_mass(raw, weights, split=split, max_edges=max_edges, depths=True)
            # multiples of 1/8 on at most 30 variables: at most 90 mantissa bits per product -- the n = 30 rows may round, the family's
            # (n <= 12) are exact, so those are equal bit for bit and the others within the derived bound
            assert np.array_equal(got[0], base[0]) and not got[3].any()
            assert (got[0].dtype, got[1].dtype, got[3].dtype, got[4].dtype, got[5].dtype) == (np.int8, np.float64, np.float64, np.int64, np.int8)
            assert np.array_equal(got[1][:122], base[1][:122]) and np.array_equal(got[1][-4:], base[1][-4:])
            assert (np.abs(got[1] - base[1]) <= 2 * zm.mass_bound(30, 1 << 17, 1.0) * base[1]).all()
            for j, (a, b) in enumerate(zip(got[2], base[2])):
                assert (a is None) == (b is None)
                if a is not None:
                    assert a.dtype == np.float64 and a.shape == b.shape
                    assert np.array_equal(a, b) if j < 122 else np.allclose(a, b, rtol=0, atol=1e-9)
            assert (got[4] >= base[4]).all() and got[4][0] == got[4][1] == got[4][-4] == got[4][-3] == got[4][-2] == got[4][-1] == 0
            assert not got[5][-3:-1].any() and got[5].max() > 0                          # more than 1023 variables: one cube
            if split == 4:
                assert (got[5][2:-4] == 4).all()
            else:
                assert (got[5] > 0).sum() >= 5 and (got[5] == 0).sum() >= 5              # some rows end in the first stage, some do not
                assert (got[4][got[5] > 0] > base[4][got[5] > 0]).all()                    # work is the sum of both stages
    assert len(exact.solution_mass(raw[:5], weights[:5], split=2)) == 5
    post = exact.solution_mass(raw[:5], weights[:5], split=2)[2]
    grad = exact.mass_logit_gradient(weights[:5], post)
    assert all(g.shape == (len(x),) for g, x in zip(grad, weights[:5])) and not grad[1].any()
    np.testing.assert_array_equal(grad[0], np.zeros(3))                                   # no clause: the posterior is the prior


def test_cli_complete_mass_split(tmp_path):
    from test_sharded_gpu import _run
    ddir = tmp_path / 'cnf'
    ddir.mkdir()
    rng = np.random.RandomState(30)
    for i in range(40):
        n, clauses = cs.threshold_3sat(rng, 30, 128)
        with open(str(ddir / ('t_%02d_0.cnf' % i)), 'w') as f:
            f.write('p cnf %d %d\n' % (n, len(clauses)) + ''.join(' '.join(str(l) for l in c) + ' 0\n' for c in clauses))
    argv = [PDP_YAML, str(ddir), '100', '-d', '--rng', 'philox', '-s', '7', '-w', '0', '--complete', '--complete-mass']
    base, _ = _run(argv, 1, str(tmp_path / 'base.jsonl'), 0)
    deep, _ = _run(argv + ['--complete-mass-split', '3'], 1, str(tmp_path / 'deep.jsonl'), 0)
    auto, _ = _run(argv + ['--complete-mass-split', '-1'], 1, str(tmp_path / 'auto.jsonl'), 0)
    assert len(base) == len(deep) == len(auto) == 40
    split = 0
    for b, d in zip(base, deep):
        r, rb = json.loads(d), json.loads(b)
        if 'mass_split_depth' not in r:
            assert d == b and rb['complete'] != 1                                        # byte-identical to the run without the flag
            continue
        assert r['mass_split_depth'] == 3 and list(r)[-2:] == ['mass_work', 'mass_split_depth']
        assert list(r)[:-1] == list(rb)
        varying = ('solution_mass', 'solution_mass_log2', 'posterior', 'mass_work', 'mass_split_depth')
        assert {k: v for k, v in r.items() if k not in varying} == {k: v for k, v in rb.items() if k not in varying}
        assert r['mass_work'] >= rb['mass_work'] and rb['solution_mass_proved'] == 1 and r['solution_mass_open'] == 0.0
        assert abs(r['solution_mass'] - rb['solution_mass']) <= 2 * zm.mass_bound(30, 1 << 17, rb['solution_mass'])
        if 'posterior' in rb:
            assert np.allclose(r['posterior'], rb['posterior'], rtol=0, atol=1e-9)
        split += 1
    assert split >= 5
    assert auto == base                                                                   # every row is weighed by the plain first stage
