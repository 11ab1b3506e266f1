"""The instances that pin the complete solvers past one wave's width (tests/exact_wide.py), on the CPU: the Python models' statistics
show that each 64-wide step of csrc/pdp_exact.hip is taken more than once -- so that test_exact_wide_gpu.py compares what it claims to --
the stats argument changes no result, the two models agree where both decide, and every model found satisfies its clauses."""
import numpy as np
import pytest

import exact_learn_model as lm
import exact_model
import exact_wide as xw
import families
from test_exact_learn_host import satisfies

LEARN_KEYS = ('trail', 'span', 'gap', 'confl_len', 'lc', 'pass_units', 'live', 'kept', 'kept_idx', 'kept_len')


def table(title, names, stats, keys):
    print(title)
    for name, s in zip(names, stats):
        print('  %-24s' % name + '  '.join('%s=%d' % (k, s.get(k, 0)) for k in keys))


@pytest.fixture(scope='module')
def fan():
    "fan(120, seed) for seeds 0, 1, 2, 4 inside the 'fan' batch: the learning model's results and statistics"
    inst, arena, budget = xw.learn_batches()['fan']
    res, stats = xw.learn_results('fan')
    at = [inst.index(f) for f in xw.fans()]
    return [inst[i] for i in at], tuple([x[i] for i in at] for x in res), [stats[i] for i in at]


def test_families_are_what_they_say():
    n, c = families.fan(120, 0)
    assert n == 221 and c[0] == [121] and c[1:101] == [[-121, 121 + i] for i in range(1, 101)] and len(c) == 101 + 511
    assert all(len(x) == 3 and len({abs(l) for l in x}) == 3 and max(abs(l) for l in x) <= 120 for x in c[101:])
    assert families.fan(120, 0) == families.fan(120, 0) != families.fan(120, 1)
    n, c = families.wide(4)
    assert n == 10 and c == [[1, 5], [2, 6], [3, 7], [4, 8]] + [[-1, -2, -3, -4, z, w] for z in (9, -9) for w in (10, -10)]
    assert families.stride((3, [[1, -2], [3]]), 5) == (11, [[1, -6], [11]])
    n, c = families.wide_kept(4)
    assert n == 12 and c[:8] == families.wide(4)[1] and c[8:] == [[-1, -2, -3, -8, z, w] for z in (11, -11) for w in (12, -12)]
    n, c = families.far_uip(2)
    assert n == 9 and c == [[-1, 2], [-1, 3], [-1, 4], [1, 7], [1, 8], [1, 9], [-2, 5], [-2, 6], [-5, -6]]


def test_fan_reaches_every_width_of_the_learning_search(fan):
    "the conditions the GPU comparison rests on, and the figures of the four runs: live 139 / 135 / 122 / 123, kept_idx 138 / 134 / 106 / 119"
    inst, res, stats = fan
    table('fan(120, seed) at arena %d, budget %d' % (xw.FAN_ARENA, xw.FAN_BUDGET), ['seed %d' % s for s in xw.FAN_SEEDS], stats, LEARN_KEYS)
    assert xw.peak(stats, 'trail') > 128
    assert xw.peak(stats, 'span') > 64
    assert xw.peak(stats, 'pass_units') > 64
    assert xw.peak(stats, 'live') > 64
    assert xw.peak(stats, 'kept') >= 1
    assert xw.peak(stats, 'kept_idx') >= 64
    assert -1 in res[0] and (1 in res[0] or 0 in res[0])
    assert [s['live'] for s in stats] == [139, 135, 122, 123] and [s['kept_idx'] for s in stats] == [138, 134, 106, 119]
    assert all(s['pass_units'] == 100 and s['trail'] >= 194 and s['span'] >= 73 for s in stats)
    e = xw.edges(inst)
    assert (np.array(res[2]) < xw.FAN_BUDGET + 4 * (e + xw.FAN_ARENA)).all()


def test_wide_reaches_long_clauses():
    "wide(D): conflict and reason clauses of D + 2 and D + 1 literals, learned clauses of D + 1 and D; the reads of both searches"
    got = {}
    for D in xw.WIDE_D:
        st, pst = {}, {}
        status, model, work, learned, red = lm.search(*families.wide(D), stats=st)
        assert status == 1 and learned == 2 and red == 0 and satisfies(families.wide(D)[1], model)
        assert st['lc'] == D + 1 > 64 and st['confl_len'] == D + 2 > 64 and st['trail'] == D + 2
        plain = exact_model.search(*families.wide(D), stats=pst)
        assert plain[0] == 1 and satisfies(families.wide(D)[1], plain[1])
        got[D] = (work, plain[2])
    assert got == {70: (63911, 62478), 100: (127271, 125238), 130: (212231, 209598)}


def test_wide_kept_keeps_a_clause_longer_than_a_wave():
    "at small_arena(D) one reduction keeps the D-literal reason of a_D (old index 1) and the search goes on to resolve with it"
    names, rows = [], []
    for D in xw.WIDE_D:
        inst, arena, _ = xw.learn_batches()['wide-%d' % D]
        res, stats = xw.learn_results('wide-%d' % D)
        for at in (inst.index(families.wide_kept(D)), len(inst) - 4):              # the instance and its strided copy
            s = stats[at]
            assert res[0][at] == 1 and res[4][at] == 1 and res[3][at] == 4
            assert s['kept_len'] == D > 64 and s['kept'] == 1 and s['kept_idx'] == 1 and s['live'] == 2 and s['confl_len'] == D + 2
            names.append('wide_kept(%d)%s' % (D, '' if at < 6 else ' strided'))
            rows.append(s)
        assert lm.search(*families.wide_kept(D), arena=arena + 2)[4] == 1          # two words more: nothing is kept (a different search)
    table('wide_kept(D) at arena 3 D + 4', names, rows, LEARN_KEYS)


def test_far_uip_steps_the_trail_scan_to_its_next_window():
    "the analysis skips exactly K trail slots between x and c, so K = 63 stays within the first window of 64 slots and K = 64 does not"
    for K in xw.FAR_K:
        st, pst = {}, {}
        inst = families.far_uip(K)
        status, model, work, learned, _ = lm.search(*inst, stats=st)
        assert status == 1 and learned == 1 and satisfies(inst[1], model)
        assert st['gap'] == K and st['pass_units'] == K + 1 and st['span'] == K + 3 and st['trail'] == K + 4
        plain = exact_model.search(*inst, stats=pst)
        assert plain[0] == 1 and pst['undone'] == K + 4 and pst['pass_units'] == K + 1
    assert 63 in xw.FAR_K and 64 in xw.FAR_K and max(xw.FAR_K) > 128


def test_fan_reaches_every_width_of_the_plain_search():
    inst = xw.plain_batch()
    res, stats = xw.plain_results(None)
    at = [inst.index(families.fan(100, s)) for s in xw.PLAIN_SEEDS]
    rows = [stats[i] for i in at]
    table('fan(100, seed), plain search, budget %d' % xw.PLAIN_BUDGET, ['seed %d' % s for s in xw.PLAIN_SEEDS], rows, ('trail', 'pass_units', 'undone'))
    assert xw.peak(rows, 'trail') > 128 and xw.peak(rows, 'pass_units') > 64 and xw.peak(rows, 'undone') > 64
    assert (res[2] < xw.PLAIN_BUDGET + 3 * xw.edges(inst)).all()
    assert {-1, 1} <= set(res[0][at].tolist())


def test_stats_change_no_result():
    for inst in (families.fan(40, 7, F=70), families.wide(70), families.far_uip(64), families.wide_kept(70)):
        for arena in (0, xw.small_arena(70)):
            a, b = lm.search(*inst, arena=arena), lm.search(*inst, arena=arena, stats={})
            assert a[0] == b[0] and a[2:] == b[2:] and np.array_equal(a[1], b[1])
        a, b = exact_model.search(*inst), exact_model.search(*inst, stats={})
        assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
    with pytest.raises(TypeError):
        lm.search(3, [[1]], None, 0, 0, {})                                        # keyword-only
    with pytest.raises(TypeError):
        exact_model.search(3, [[1]], None, 0, {})


def test_stride_changes_positions_only():
    "a monotone renumbering: status, work, learned, reductions and the statistics stay, the model moves to the new ids"
    for name in xw.learn_batches():
        inst, arena, budget = xw.learn_batches()[name]
        res, stats = xw.learn_results(name)
        pairs = [(i, j) for i, a in enumerate(inst) for j, b in enumerate(inst)
                 if i != j and any(families.stride(a, s) == b for s in (3, xw.STRIDE))]
        assert len(pairs) == 2
        for i, j in pairs:
            s = (xw.sizes(inst)[j] - 1) // (xw.sizes(inst)[i] - 1)
            assert all(res[k][i] == res[k][j] for k in (0, 2, 3, 4)) and stats[i] == stats[j]
            assert np.array_equal(res[1][j][::s], res[1][i]) and res[1][j].sum() == res[1][i].sum()


def test_models_agree_and_satisfy():
    "every status-1 model satisfies its clauses; where both models decide an instance they give one status"
    for name in xw.learn_batches():
        inst = xw.learn_batches()[name][0]
        res, _ = xw.learn_results(name)
        assert all(satisfies(c, m) if s == 1 else not m.any() for (n, c), s, m in zip(inst, res[0], res[1]))
    inst = xw.plain_batch()
    plain, _ = xw.plain_results(None)
    learn, _ = xw.plain_learn_results(None)
    for res in (plain, learn):
        assert all(satisfies(c, m) if s == 1 else not m.any() for (n, c), s, m in zip(inst, res[0], res[1]))
    both = (plain[0] != -1) & (learn[0] != -1)
    assert both.sum() >= len(inst) - 2
    np.testing.assert_array_equal(plain[0][both], learn[0][both])
    # the fan(120) set: the plain model on what the learning model decided
    f, (res, _) = xw.fans(), xw.learn_results('fan')
    binst = xw.learn_batches()['fan'][0]
    for inst_ in f:
        s = res[0][binst.index(inst_)]
        if s != -1:
            p = exact_model.search(*inst_, budget=xw.FAN_BUDGET)
            assert p[0] in (-1, s)
