"""The device math of include/pdp_math.h on EVERY float32 input (2^32 per single-argument function, a second or so on the MI355X).

The kernels and the oracle share the header, but not its code: on the device pdp_scale2 is v_ldexp_f32, pdp_safe_log_fin splits with
v_frexp_*, pdp_fmaxf / pdp_fminf are v_max_f32 / v_min_f32 and pdp_rcp_ge1 (inside sigmoid and tanh_abs) is v_rcp_f32 plus Newton steps,
where the host has products, bit moves, selects and a division.  Three statements, none of them sampled (measured: about a second per
checksum case, under a second for every other case):
  * every output bit of every probe is the oracle's (per-block checksums recorded by tools/math_checksums.py);
  * the accuracy figures of the header hold against float64, and the worst cases are the oracle's;
  * the lean and select-free forms are the general ones on their domains, and both tanh forms are odd.
tests/math_sweep.py holds the statements; tests/test_math_sweep_host.py checks them for the oracle on a fixed set of blocks."""
import time

import numpy as np
import pytest
import torch

import math_sweep as ms

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24                          # inputs per launch: four blocks, well under 2 GB of temporaries
assert CHUNK % ms.BLOCK == 0 and (1 << 32) % CHUNK == 0


@pytest.fixture(scope='module')
def ops():
    return ms.TorchOps(torch.device('cuda:0'))


@pytest.fixture(scope='module')
def recorded():
    return ms.load_fixture()


def _apply():
    from pdp import native
    return native.math_apply


def _apply_one(ops):
    apply = _apply()
    return lambda fn, v: int(ops.out_bits(apply(fn, torch.tensor([v], dtype=torch.float32, device=ops.device)))[0].item())


def _done(what, t0):
    torch.cuda.synchronize()
    print('%s: 2^32 inputs in %.2f s' % (what, time.time() - t0))


@pytest.mark.parametrize('probe', ms.PROBES)
def test_every_input_equals_the_oracle(oracle, ops, recorded, probe):
    apply, t0 = _apply(), time.time()
    want = torch.from_numpy(recorded[ms.PROBES.index(probe)].view(np.int64)).to(ops.device)          # every sum is below 2^63
    w = ops.weights()
    differs = torch.zeros(ms.N_BLOCKS, dtype=torch.bool, device=ops.device)
    compared = 0
    for start in range(0, 1 << 32, CHUNK):
        y = apply(probe, ops.as_float(ops.input_bits(start, CHUNK)))
        k0, k1 = start // ms.BLOCK, (start + CHUNK) // ms.BLOCK
        differs[k0:k1] = (ms.checksum(ops, y, w) != want[k0:k1]).any(1)
        compared += k1 - k0
        del y
    assert compared == ms.N_BLOCKS
    bad = torch.nonzero(differs).reshape(-1).tolist()
    _done('%s against the recorded oracle' % probe, t0)
    if bad:
        start = bad[0] * ms.BLOCK
        got = ms.NumpyOps().out_bits(apply(probe, ops.as_float(ops.input_bits(start, ms.BLOCK))).cpu().numpy())
        npo = ms.NumpyOps()
        ref = npo.out_bits(oracle.math_apply(probe, npo.as_float(npo.input_bits(start, ms.BLOCK))))
        d = np.nonzero(got != ref)[0]
        where = ('first differing input 0x%08x: device 0x%08x, oracle 0x%08x; %d in that block'
                 % (start + int(d[0]), int(got[d[0]]), int(ref[d[0]]), d.size)) if d.size else \
            'the live oracle agrees with the device on that block: tests/golden/math_checksums.npz is stale (tools/math_checksums.py)'
        pytest.fail('%s: %d of %d blocks differ from the recorded oracle, the first from 0x%08x; %s' % (probe, len(bad), ms.N_BLOCKS, start, where))


@pytest.mark.parametrize('fn', ms.ACCURACY_FUNCTIONS)
def test_accuracy_against_float64_on_every_input(ops, fn):
    """the header's figures (exp, log < 1.5 ulp; logsigmoid < 3 ulp; tanh_abs < 1.2e-7), those of test_math_accuracy (sigmoid 1.5e-7, tanh
    2e-7 absolute), the special values, and for sigmoid and tanh the oracle's measured relative maxima rounded up to the next half ulp
    (2.5 and 3.0); the reference is torch float64 on the device"""
    apply, t0 = _apply(), time.time()
    tally = ms.Tally(fn, _apply_one(ops))
    for start in range(0, 1 << 32, CHUNK):
        tally.add(ops, start, apply(fn, ops.as_float(ops.input_bits(start, CHUNK))))
    _done('%s against float64' % fn, t0)
    print('\n'.join(tally.report()))
    assert tally.seen == 1 << 32
    tally.check()
    for (f, kind, name), (xb, err) in ms.ORACLE_WORST.items():
        if f == fn:                                           # the device's bits are the oracle's: so is its worst case
            e, at, _ = tally.worst[(kind, name)]
            assert ms.same_input(fn, at, xb) and ms.same_figure(e, err), '%s, %s: worst %.5g at 0x%08x, the oracle has %.5g at 0x%08x' % (fn, name, e, at, err, xb)


@pytest.mark.parametrize('relation', ms.LEAN_FORMS, ids=[r[0] + '-' + r[1] for r in ms.LEAN_FORMS])
def test_lean_forms_equal_the_general_forms_on_every_input(ops, relation):
    apply, t0 = _apply(), time.time()
    total, first = 0, None
    for start in range(0, 1 << 32, CHUNK):
        cnt, xb, a, g = ms.lean_mismatches(ops, apply, relation, start, CHUNK)
        total += cnt
        first = first or ((xb, a, g) if cnt else None)
    _done('%s against %s' % relation[:2], t0)
    assert total == 0, '%d inputs; first: %s(0x%08x) = 0x%08x, %s gives 0x%08x' % ((total, relation[0]) + first[:2] + (relation[1], first[2]))


@pytest.mark.parametrize('fn', ['tanh', 'tanh_abs'])
def test_tanh_forms_are_odd_on_every_input(ops, fn):
    apply, t0 = _apply(), time.time()
    total, first = 0, None
    for start in range(0, 1 << 31, CHUNK):
        cnt, xb, p, m = ms.odd_mismatches(ops, apply, fn, start, CHUNK)
        total += cnt
        first = first or ((xb, p, m) if cnt else None)
    _done('%s(-x) against %s(x)' % (fn, fn), t0)
    assert total == 0, '%d inputs; first: %s(0x%08x) = 0x%08x but 0x%08x for -x' % ((total, fn) + (first or (0, 0, 0)))
