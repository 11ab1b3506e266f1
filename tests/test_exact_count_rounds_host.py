"""The resumable counting search without a GPU: its Python statement (tests/exact_count_rounds_model.py) run until the frontier is empty
against the plain counting search's (tests/exact_count_model.py) and brute force, for budgets and gives that stop it at every node;
caller-made frontiers of closed paths, which pin the leaf inside a path; the progress rule; the work bound; the refusals; the header."""
import functools
import itertools
import os
import re

import numpy as np
import pytest

import exact_count_cases as cs
import exact_count_model as cm
import exact_count_rounds_model as rm
from helpers import REPO

PAIRS = [(1, 0), (1, 3), (40, 1), (200, 8)]            # reads per cube and round, levels given away per stopped cube


@functools.lru_cache(maxsize=None)
def plain():
    return [cm.search(n, c) for n, c in cs.family()]


def node_bound(n, clauses):
    "the reads of one node: at most n + 1 propagation passes of at most e reads each, and a branching pass of at most 2 e"
    e = sum(len(c) for c in clauses)
    return (n + 3) * e


@pytest.mark.parametrize('budget,give', PAIRS)
def test_rounds_add_up_to_the_plain_count(budget, give):
    fam, want, brute = cs.family(), plain(), cs.family_brute()
    assert len(fam) >= 400
    state = rm.State(fam)
    rounds = 0
    while state.cubes():
        before = [list(p) for p in state.paths]
        rec = rm.round(fam, state, budget, give)
        rounds += 1
        flat = [p for ps in before for p in ps]
        assert len(rec) == len(flat)
        for path, (b, st, count, work, leaves, replay, cp) in zip(flat, rec):
            n, clauses = fam[b]
            assert (st == 1) == (cp is None) and cp != path                       # no round returns its checkpoint unchanged
            assert replay <= work <= replay + budget + node_bound(rm.inst_n(fam[b]), clauses)
            assert st == 1 or work - replay >= budget
            if cp is not None:
                rm.check_path(rm.inst_n(fam[b]), cp)
    for b, w in enumerate(want):
        assert (state.count[b], state.leaves[b]) == (w[1], w[4]) and state.count[b] == brute[b][0], b
        np.testing.assert_array_equal(state.true_count[b], w[2])
        assert state.true_count[b].tolist() == brute[b][1].tolist()
        assert state.work[b] >= w[3]                                              # paths are replayed
    assert state.status() == [1] * len(fam)
    assert rounds == max(state.rounds) and (rounds > 100) == ((budget, give) == (1, 0))
    print('budget %d give %d: %d rounds, reads %.2f times the plain count' % (budget, give, rounds, sum(state.work) / sum(w[3] for w in want)))


@pytest.mark.parametrize('n,ratio,budget,give', [(20, 3.5, 3000, 0), (20, 3.5, 3000, 4), (30, 4.0, 5000, 0), (30, 4.0, 3000, 8)])
def test_uniform_3sat(n, ratio, budget, give):
    inst = cs.uniform_3sat(n + give, n, (ratio,), 2)
    state = rm.run(inst, budget, give)
    for b, (k, c) in enumerate(inst):
        w = cm.search(k, c)
        assert (state.count[b], state.leaves[b]) == (w[1], w[4])
        np.testing.assert_array_equal(state.true_count[b], w[2])
    assert max(state.rounds) > 1


def finish(n, clauses, paths, budget, give):
    "the counts of a caller-made frontier, run until it is empty"
    count, leaves, tc = 0.0, 0, np.zeros(n)
    while paths:
        nxt = []
        for p in paths:
            st, c, t, _, lv, _, cp = rm.cube(n, clauses, p, budget)
            count, leaves, tc = count + c, leaves + lv, tc + t
            if st == -1:
                nxt += rm.children(cp, give)
        paths = nxt
    return count, leaves, tc


@pytest.mark.parametrize('depth', [1, 2, 3, 4, 5])
def test_closed_paths_of_every_depth_add_up(depth):
    # 2^depth paths of closed levels are pdp_exact_count_split's cubes: where the tree is shallower than the path, a leaf is met by every
    # path that shares its levels' bits, and counted by the one whose remaining bits are 0
    fam, want = cs.family()[::4], plain()[::4]
    inside = 0
    for (n, c), w in zip(fam, want):
        n = rm.inst_n((n, c))
        if depth > n:
            continue
        paths = [[(b, 1) for b in bits] for bits in itertools.product((0, 1), repeat=depth)]
        for budget, give in ((1 << 30, 0), (60, 1)):
            count, leaves, tc = finish(n, c, paths, budget, give)
            assert (count, leaves) == (w[1], w[4])
            np.testing.assert_array_equal(tc, w[2])
        empty = [p for p in paths if rm.cube(n, c, p, 1 << 30)[4] == 0]
        inside += len(empty) > 0 and w[4] > 0
    assert inside > 10


def test_open_levels_of_a_caller_made_path():
    # (0, 0) on every level is the root cube met later: the same count; (0, 1) on level 1 leaves out the other half of the tree
    n, clauses = cs.uniform_3sat(5, 16, (3.0,), 1)[0]
    w = cm.search(n, clauses)
    assert finish(n, clauses, [[(0, 0)] * 3], 100, 2)[:2] == (w[1], w[4])
    half = finish(n, clauses, [[(0, 1)]], 100, 2)
    other = finish(n, clauses, [[(1, 1)]], 100, 2)
    assert half[0] + other[0] == w[1] and half[1] + other[1] == w[4] and 0 < half[0] < w[1]
    np.testing.assert_array_equal(half[2] + other[2], w[2])


def test_children_partition_the_checkpoint():
    cp = [(0, 0), (1, 1), (0, 0), (0, 1), (0, 0)]
    assert rm.children(cp, 0) == [cp]
    assert rm.children(cp, 2) == [[(1, 1)], [(0, 1), (1, 1), (1, 1)], [(0, 1), (1, 1), (0, 1), (0, 1), (0, 0)]]
    assert rm.children(cp, 9) == [[(1, 1)], [(0, 1), (1, 1), (1, 1)], [(0, 1), (1, 1), (0, 1), (0, 1), (1, 1)],
                                  [(0, 1), (1, 1), (0, 1), (0, 1), (0, 1)]]
    ln, bits, closed = rm.pack(rm.children(cp, 2), 2)
    assert ln.tolist() == [1, 3, 5] and bits.tolist() == [[1, 0], [6, 0], [2, 0]] and closed.tolist() == [[1, 0], [7, 0], [15, 0]]
    assert rm.unpack(ln, bits, closed) == rm.children(cp, 2)
    assert rm.words(0) == rm.words(32) == 1 and rm.words(33) == 2 and rm.words(1023) == 32


def test_refusals():
    n, clauses = 4, [[1, 2], [-1, 3], [2, -4]]
    for path in ([(1, 0)], [(0, 1), (1, 0)], [(0, 0)] * 5):
        with pytest.raises(ValueError):
            rm.cube(n, clauses, path, 10)
    state = rm.State([(n, clauses), (1024, [[1, 2], [-1, 1024]])])
    assert state.paths == [[[]], []] and state.status() == [-1, -2]
    rm.run([(n, clauses), (1024, [[1, 2], [-1, 1024]])], 5, 1)
    assert rm.cube(n, clauses, [], 0)[0] == 1                                     # budget <= 0: the default, far above this tree


def test_header_and_symbols():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = re.sub(r'\s+', ' ', f.read())
    assert '#define PDP_ABI_VERSION 3' in text and '#define PDP_EXACT_ROUND_BUDGET (((int64_t)1) << 18)' in text
    assert "int pdp_exact_count_frontier_words(pdp_problem *p, int32_t *words_host);" in text
    assert ("int pdp_exact_count_round(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int32_t *len, const uint32_t *bits, "
            "const uint32_t *closed, int64_t budget, double *count, double *true_count, int64_t *work, int64_t *leaves, int8_t *cube_status, "
            "int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out, double *cube_count, int64_t *cube_work, int64_t *cube_leaves, "
            "int64_t *cube_replay, void *stream);") in text
    assert ("int pdp_exact_count_expand(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int8_t *cube_status, const int32_t *len, "
            "const uint32_t *bits, const uint32_t *closed, int32_t give, int64_t capacity, int64_t *cube_off_new, int32_t *len_new, "
            "uint32_t *bits_new, uint32_t *closed_new, int64_t *cubes_new_host, void *stream);") in text
    from pdp import exact, native
    assert {'pdp_exact_count_frontier_words', 'pdp_exact_count_round', 'pdp_exact_count_expand'} <= set(native.EXPORTED_SYMBOLS)
    assert exact.ROUND_BUDGET == rm.ROUND_BUDGET == 1 << 18 and native.COUNT_ROUNDS_MAX_CUBES == rm.MAX_CUBES
    assert {'cube_off', 'len', 'bits', 'closed', 'count', 'true_count', 'work', 'leaves', 'status', 'rounds'} == set(native.CountState.FIELDS)


@pytest.mark.parametrize('kw', [dict(split='rounds', round_budget=0), dict(split='rounds', rounds=-1), dict(split='rounds', round_budget=1.5),
                                dict(split=3, rounds=2), dict(round_budget=5)])
def test_count_models_refuses_bad_rounds(kw):
    from pdp import exact
    with pytest.raises(ValueError, match='round'):
        exact.count_models([exact.raw_item(2, [[1, 2]])], **kw)
