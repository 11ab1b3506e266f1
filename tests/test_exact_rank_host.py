"""The k-th model of the counting complete search without a GPU: its Python statement (tests/exact_rank_model.py) against brute-force
enumeration and the counting statement, its three consequences (enumeration, the count's work, answers that depend on the rank alone),
duplicates, no ranks, ranks inside a leaf wider than 2^53, instances that are too large, the header, and exact.sample_models' draw."""
import os
import re

import numpy as np

import exact_count_cases as cs
import exact_count_model as cm
import exact_rank_cases as rc
import exact_rank_model as rm
from helpers import REPO


def test_all_ranks_enumerate_the_models():
    "(a) and (b): ranks 0 .. count give the brute-force model set, each model once, with the counting search's work, leaves and count"
    inst, counts = cs.family(), rc.family_counts()
    assert len(inst) >= 300 and max(n for n, _ in inst) <= 12
    some = 0
    for (n, c), ranks, (cst, count, tc, cwork, cleaves), (bc, _) in zip(inst, rc.family_ranks(), counts, cs.family_brute()):
        st, seen, found, models, work, leaves = rm.search(n, c, ranks)
        assert cst == 1 and count == bc and len(ranks) == bc + 1
        assert (st, seen, work, leaves) == (1, count, cwork, cleaves)
        assert found.dtype == np.int8 and models.dtype == np.uint8 and models.shape == (bc + 1, len(tc))
        assert found.tolist() == [1] * bc + [0] and not models[bc].any()
        rows = [r.tobytes() for r in models[:bc]]
        assert len(set(rows)) == bc and set(rows) == rc.brute_models(n, c)
        np.testing.assert_array_equal(models[:bc].sum(axis=0, dtype=np.int64).astype(np.float64), tc)       # bit for bit: exact integers
        some += bc > 1
    assert some > 200


def test_answers_depend_on_the_rank_alone():
    "(b) and (c): any subset of ranks gives the same rows with no more work; a smaller budget answers with the same model or with -1"
    rng = np.random.RandomState(5)
    inst, counts, all_ranks = cs.family(), rc.family_counts(), rc.family_ranks()
    seen_status, seen_found = set(), set()
    for j in range(0, len(inst), 3):
        (n, c), ranks, (_, count, _, cwork, cleaves) = inst[j], all_ranks[j], counts[j]
        full = rm.search(n, c, ranks)
        k = int(rng.randint(1, 6))
        sub = sorted(int(r) for r in rng.choice(len(ranks), size=k))                      # with repeats; may hold the rank beyond
        st, seen, found, models, work, leaves = rm.search(n, c, [ranks[i] for i in sub])
        assert st == 1 and work <= cwork and leaves <= cleaves and seen <= count
        if ranks[sub[-1]] >= count:
            assert (work, leaves, seen) == (cwork, cleaves, count)
        np.testing.assert_array_equal(found, full[2][sub])
        np.testing.assert_array_equal(models, full[3][sub])
        edges = sum(len(x) for x in c)
        for budget in (1, 50, 500, 5000):
            bst, bseen, bfound, bmodels, bwork, bleaves = rm.search(n, c, ranks, budget)
            assert bwork < budget + 3 * edges and bwork <= full[4] and bleaves <= full[5] and bseen <= full[1]
            assert (bst == 1) == (bwork == full[4] and (bfound != -1).all())
            if bst == -1:
                assert bwork >= budget
                cut = int((bfound == 1).sum())
                assert bfound.tolist() == [1] * cut + [-1] * (len(ranks) - cut)           # non-decreasing ranks: answered ones come first
            answered = bfound == 1
            np.testing.assert_array_equal(bmodels[answered], full[3][answered])
            assert not bmodels[~answered].any()
            seen_status.add(bst)
            seen_found |= set(bfound.tolist())
    assert seen_status == {1, -1} and seen_found == {1, 0, -1}


def test_duplicates_and_no_ranks():
    n, c = 4, [[1, 2], [-1, 3]]
    count = cm.search(n, c)[1]
    assert count == 8.0
    full = rm.search(n, c, list(range(9)))
    ranks = [0, 0, 3, 3, 3, 7, 8, 8]
    st, seen, found, models, work, leaves = rm.search(n, c, ranks)
    assert st == 1 and found.tolist() == [1] * 6 + [0, 0] and (work, leaves, seen) == (full[4], full[5], 8.0)
    np.testing.assert_array_equal(models, full[3][ranks])
    for n, c in ((4, [[1, 2], [-1, 3]]), (2, [[1], [-1]]), (3, [])):
        st, seen, found, models, work, leaves = rm.search(n, c, [])
        assert (st, seen, work, leaves) == (1, 0.0, 0, 0) and found.shape == (0,) and models.shape == (0, n)
    # unsatisfiable: every rank is "no such model"
    st, seen, found, models, work, leaves = rm.search(2, [[1], [-1]], [0, 1, rc.TOP])
    assert st == 1 and seen == 0.0 and found.tolist() == [0, 0, 0] and not models.any() and work == cm.search(2, [[1], [-1]])[3]
    # rank 0 alone stops at the first leaf
    n, c = cs.uniform_3sat(9, 20, (3.0,), 1)[0]
    cst, count, _, cwork, cleaves = cm.search(n, c)
    st, seen, found, models, work, leaves = rm.search(n, c, [0])
    assert count > 1 and st == 1 and found.tolist() == [1] and leaves == 1 and work < cwork and seen <= count
    assert rc.satisfied(models, c).all()


def test_ranks_inside_a_wide_leaf():
    "the fans: count 2^k + 1, the first leaf has x1 true and all k y's free; ranks 0, 5 and 2^53 - 1 set 0, 2 and 53 of them"
    for k in cs.FAN_K:
        n, c = cs.fan(k)
        ranks = [0, 5, rc.TOP]
        st, seen, found, models, work, leaves = rm.search(n, c, ranks)
        assert st == 1 and found.tolist() == [1, 1, 1] and leaves == 1 and seen == 2.0 ** k and work <= cm.search(n, c)[3]
        assert models[:, 0].tolist() == [1, 1, 1] and models[:, 1:].sum(axis=1).tolist() == [0, 2, 53]
        for r, row in zip(ranks, models):
            assert row[1:].tolist() == rc.bits(r, 53) + [0] * (k - 53)
        assert rc.satisfied(models, c).all()


def test_free_variables_take_the_bits_in_ascending_index():
    n, c = rc.fixed_prefix()
    st, seen, found, models, _, leaves = rm.search(n, c, rc.PATTERNS)
    assert st == 1 and seen == 2.0 ** 40 and leaves == 1 and (found == 1).all()
    for r, row in zip(rc.PATTERNS, models):
        assert row[:70].tolist() == [1, 0] * 35 and row[70:].tolist() == rc.bits(r, 40)
    n, c = rc.fixed_evens()
    st, seen, found, models, _, _ = rm.search(n, c, rc.WIDE_RANKS)
    assert st == 1 and seen == 2.0 ** 65 and (found == 1).all()
    for r, row in zip(rc.WIDE_RANKS, models):
        assert row[1::2].tolist() == [1] * 65 and row[0::2].tolist() == rc.bits(r, 53) + [0] * 12


def test_too_many_variables():
    st, seen, found, models, work, leaves = rm.search(1024, [[1, 2], [-1, 1024]], [0, 3])
    assert (st, seen, work, leaves) == (-2, 0.0, 0, 0) and found.tolist() == [-1, -1] and models.shape == (2, 1024) and not models.any()
    st, seen, found, models, _, _ = rm.search(1023, [[1, 2], [-1, 1023]], [0, rc.TOP])
    assert st == 1 and found.tolist() == [1, 1] and rc.satisfied(models, [[1, 2], [-1, 1023]]).all()


def test_header_and_symbol():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = f.read()
    assert '#define PDP_ABI_VERSION 3' in text
    proto = ("int pdp_exact_models_at(pdp_problem *p, const int64_t *rank_off, const int64_t *ranks, int64_t budget, int8_t *status, "
             "double *count_seen, int8_t *found, uint8_t *models, int64_t *work, int64_t *leaves, void *stream);")
    assert proto in re.sub(r'\s+', ' ', text)
    from pdp import native
    assert 'pdp_exact_models_at' in native.EXPORTED_SYMBOLS


SAMPLE_SEED = 0


def test_the_draw_of_sample_models_is_uniform_over_the_models():
    """exact.sample_models' ranks on the Python model, k = 4096 on an instance of at most 4096 models: every row is a model and every
    variable's sample mean lies within 5 sigma (+ 1/k) of its exact marginal.  The draw is seeded, so the outcome is fixed."""
    from pdp import exact
    k = 4096
    rng = np.random.RandomState(16)
    while True:
        n, c = cs.threshold_3sat(rng, 18, 66)
        st, count, tc, _, _ = cm.search(n, c)
        if 200 <= count <= 4096:
            break
    ranks = exact.sample_ranks(count, k, SAMPLE_SEED, 0)
    assert ranks.shape == (k,) and ranks.min() >= 0 and ranks.max() < count
    np.testing.assert_array_equal(ranks, exact.sample_ranks(count, k, SAMPLE_SEED, 0))
    assert not np.array_equal(ranks, exact.sample_ranks(count, k, SAMPLE_SEED, 1))        # the instance's index is part of the key
    order = np.argsort(ranks, kind='stable')
    st, _, found, models, _, _ = rm.search(n, c, ranks[order])
    assert st == 1 and (found == 1).all() and rc.satisfied(models, c).all()
    sample = np.empty_like(models)
    sample[order] = models
    p = tc / count
    mean = sample.mean(axis=0)
    bound = 5.0 * np.sqrt(p * (1.0 - p) / k) + 1.0 / k
    print('sample of %d from %d models: largest |mean - p| / bound = %.3f' % (k, int(count), float(np.max(np.abs(mean - p) / bound))))
    assert (np.abs(mean - p) <= bound).all()
    assert len({r.tobytes() for r in sample}) > min(int(count), k) // 3                   # many different models, not a few
