"""The weighted counting search without a GPU: its Python statement (tests/exact_mass_model.py) against exact rational arithmetic, against
the counting search's statement at weights 0.5, the zero-mass pruning, 0/1 weights, the budget's bracket, the order of the products, the
refused instances, and the header."""
import os
import re
from fractions import Fraction

import numpy as np

import exact_count_cases as cs
import exact_count_model as cm
import exact_mass_cases as zc
import exact_mass_model as zm
import exact_model
from helpers import REPO


def test_model_equals_rational_arithmetic_on_eighths():
    inst, weights = zc.small()
    want = zc.small_brute()
    assert len(inst) >= 150 and max(zc.size(i) for i in inst) <= 10
    assert {float(x) for w in weights for x in w} == {k / 8.0 for k in range(9)}
    zero = sum(1 for z, _ in want if z == 0)
    print('eighths: %d instances, %d with mass 0' % (len(inst), zero))
    assert 4 * zero >= len(inst) and 4 * (len(inst) - zero) >= len(inst)
    for (n, c), w, (z, true) in zip(inst, weights, want):
        st, mass, tm, open_mass, work, leaves = zm.search(n, c, w)
        assert st == 1 and open_mass == 0.0 and tm.dtype == np.float64 and tm.shape == (zc.size((n, c)),)
        assert Fraction(mass) == z and [Fraction(float(x)) for x in tm] == true          # equal: at most 30 mantissa bits per product
        assert (leaves > 0) == (z > 0)


def test_random_weights_within_the_derived_bound():
    inst = zc.small()[0]
    worst_z = worst_t = 0.0
    for (n, c), w in zip(inst, zc.small_random()):
        n = zc.size((n, c))
        z, true = zc.brute(n, c, w)
        st, mass, tm, open_mass, work, leaves = zm.search(n, c, w)
        assert st == 1 and open_mass == 0.0
        ez = abs(Fraction(mass) - z)
        et = max(abs(Fraction(float(x)) - t) for x, t in zip(tm, true))
        assert ez <= Fraction(zm.mass_bound(n, leaves, 1.0)) * z, (n, c, w.tolist())
        assert et <= Fraction(zm.true_mass_bound(n, leaves, 1.0)) * z, (n, c, w.tolist())
        if z > 0:
            unit = Fraction((n + leaves) * zm.U) * z
            worst_z, worst_t = max(worst_z, float(ez / unit)), max(worst_t, float(et / unit))
    print('random weights: worst |Z - Z*| = %.3f, worst |true_mass - exact| = %.3f, in units of (n + leaves) u Z*' % (worst_z, worst_t))


def test_half_weights_are_the_counting_search():
    inst = cs.family() + [cs.fan(k) for k in cs.FAN_K]
    assert len(cs.family()) >= 400
    for n, c in inst:
        n = zc.size((n, c))
        st, count, tc, work, leaves = cm.search(n, c)
        zst, mass, tm, open_mass, zwork, zleaves = zm.search(n, c, zc.half(n))
        assert (zst, zwork, zleaves, open_mass) == (st, work, leaves, 0.0)
        assert mass * 2.0 ** n == count and np.array_equal(tm * 2.0 ** n, tc)


def test_the_pruning_changes_no_bit():
    less = 0
    for (n, c), w in zip(*zc.small()):
        a, b = zm.search(n, c, w), zm.search(n, c, w, prune=False)
        assert a[0] == b[0] == 1 and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3] == 0.0
        assert a[4] <= b[4] and a[5] <= b[5]
        less += a[4] < b[4]
    assert less >= 50                                                                     # the rule is at work


def test_zero_one_weights():
    inst = [i for i in cs.family() if cm.search(*i)[1] > 0] + [i for i, _ in zc.satisfiable_3sat(17, 20, (3.5, 4.0), 4)]
    many = 0
    for n, c in inst:
        n = zc.size((n, c))
        st, model, _ = exact_model.search(n, c)
        assert st == 1
        w = np.asarray(model, dtype=np.float32)
        zst, mass, tm, open_mass, work, leaves = zm.search(n, c, w)
        assert (zst, mass, open_mass, leaves) == (1, 1.0, 0.0, 1) and np.array_equal(tm / mass, w.astype(np.float64))
        count = cm.search(n, c)
        if count[4] > 1:
            assert work < count[3]
            many += 1
        clause = next((k for k in c if k and not any(-l in k for l in k)), None)
        if clause is not None:
            for l in clause:                                                              # every literal of one clause false: not a model
                w[abs(l) - 1] = 0.0 if l > 0 else 1.0
            zst, mass, tm, open_mass, work, leaves = zm.search(n, c, w)
            assert (zst, mass, open_mass, leaves) == (1, 0.0, 0.0, 0) and not tm.any()
    assert many >= 50


BUDGETS = (1, 2000, 10000, 50000)


def test_budget_brackets_the_mass():
    cases = zc.satisfiable_3sat(630, 30, (3.0, 3.5, 4.0), 2)
    fired = set()
    first_pass_decides_nothing = 0
    for (n, c), model in cases:
        edges = sum(len(k) for k in c)
        for conf in (0.5, 0.7, 0.9, 0.99):
            w = zc.around(model, conf)
            full = zm.search(n, c, w)
            assert full[0] == 1 and full[1] > 0
            last = 0.0
            for budget in BUDGETS:
                got = zm.search(n, c, w, budget)
                st, mass, tm, open_mass, work, leaves = got
                # -1 exactly where the check fired: a run the budget never stopped is the complete one
                assert st in (1, -1) and work < budget + 3 * edges
                if st == -1:
                    assert work >= budget and leaves <= full[5]
                else:
                    assert (mass, open_mass, work, leaves) == (full[1], 0.0, full[4], full[5]) and np.array_equal(tm, full[2])
                if full[4] < budget:
                    assert st == 1
                assert mass >= last
                last = mass
                zc.check_bracket(n, got, full[1], full[5])
                fired.add(st)
                if budget == 1:
                    # 3-SAT: the first pass meets no unit, so nothing is decided when the budget check fires
                    assert (st, mass, open_mass, leaves) == (-1, 0.0, 1.0, 0)
                    first_pass_decides_nothing += 1
    assert -1 in fired and first_pass_decides_nothing == 24


def test_the_product_order_is_the_butterfly_of_ascending_chunks():
    k = 150
    n, clauses = cs.fan(k)
    rng = np.random.RandomState(150)
    w = rng.uniform(0.5, 1.0, size=n).astype(np.float32)
    w[0] = 0.0                                        # x1 false first, which forces all 150 on one level; x1 true has no mass: Z is that leaf
    st, mass, tm, open_mass, work, leaves = zm.search(n, clauses, w)
    assert (st, leaves, open_mass) == (1, 1, 0.0)
    p = [float(x) for x in w]
    forced = p[1:]                                                                        # the y_i are forced true, in variable order
    first = 1.0 - p[0]
    for base in range(0, k, 64):
        first = first * zm.chunk_product(forced[base:base + 64])
    assert mass == first > 0.0
    left = 1.0 - p[0]
    for x in forced:
        left = left * x
    whole = 1.0 - p[0]
    pair = list(forced)
    while len(pair) > 1:                                                                  # one tree over all 150 instead of three chunks
        pair = [pair[i] * pair[i + 1] if i + 1 < len(pair) else pair[i] for i in range(0, len(pair), 2)]
    whole = whole * pair[0]
    assert first != left and first != whole                                              # the weights tell the orders apart


def test_refused_instances():
    n = 1024
    st, mass, tm, open_mass, work, leaves = zm.search(n, [[1, 2], [-1, 1024]], zc.half(n))
    assert (st, mass, open_mass, work, leaves) == (-2, 0.0, 0.0, 0, 0) and tm.shape == (n,) and not tm.any()
    assert zm.search(1023, [[1, 2], [-1, 1023]], zc.half(1023))[:2] == (1, 0.5)
    for bad in (np.nan, 1.5, -0.1):
        w = np.array([0.25, bad, 0.75], dtype=np.float32)
        st, mass, tm, open_mass, work, leaves = zm.search(3, [[1, 2], [-2, 3]], w)
        assert (st, mass, open_mass, work, leaves) == (-3, 0.0, 0.0, 0, 0) and tm.shape == (3,) and not tm.any()
    assert zm.search(3, [[1, 2], [-2, 3]], np.array([0.0, 1.0, 1.0], dtype=np.float32))[:2] == (1, 1.0)


def test_header_and_symbol():
    with open(os.path.join(REPO, 'include', 'pdp_hip.h')) as f:
        text = f.read()
    assert '#define PDP_ABI_VERSION 3' in text
    proto = ("int pdp_exact_mass(pdp_problem *p, const float *weights, int64_t budget, int8_t *status, double *mass, double *true_mass, "
             "double *open_mass, int64_t *work, int64_t *leaves, void *stream);")
    assert proto in re.sub(r'\s+', ' ', text)
    from pdp import native
    assert 'pdp_exact_mass' in native.EXPORTED_SYMBOLS
    assert hasattr(native.lib(), 'pdp_exact_mass')
