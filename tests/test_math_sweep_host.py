"""CPU side of the exhaustive math sweep (tests/math_sweep.py): the recorded checksums of the oracle (tests/golden/math_checksums.npz,
written by tools/math_checksums.py) still describe the header as it is, and the statements that tests/test_math_sweep_gpu.py makes about
every input hold for the oracle on a fixed set of blocks: those around the special values and thresholds of the header, eight random
ones and those of the recorded worst cases.  The exhaustive run of the oracle is tools/math_checksums.py [--accuracy]."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import math_sweep as ms

OPS = ms.NumpyOps()

NAMED = (0x00000000, 0x00800000, 0x3f3504f3, 0x3f800000, 0x41f00000, 0x42b17218, 0xc2d00000, 0x7f800000, 0x80000000, 0xff800000, 0xffffffff)


def _sample_blocks():
    ks = [ms.block_of(b) for b in NAMED]
    assert len(set(ks)) == len(NAMED)
    for k in np.random.RandomState(0).permutation(ms.N_BLOCKS):
        if len(ks) == len(NAMED) + 8:
            break
        if int(k) not in ks:
            ks.append(int(k))
    return sorted(ks)


SAMPLE = _sample_blocks()


@pytest.fixture(scope='module')
def pool():
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:          # ctypes releases the GIL
        yield ex


@pytest.fixture(scope='module')
def apply(oracle):
    """oracle.math_apply with the array cut into slices that run side by side: a block of denormal inputs or results takes the CPU
    thirty times as long as any other, and would otherwise keep one thread busy while the rest have finished"""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as inner:          # not `pool`: its tasks wait for these
        def run(fn, x):
            n = max(1, x.size // 8)
            return np.concatenate(list(inner.map(lambda i: oracle.math_apply(fn, x[i:i + n]), range(0, x.size, n))))
        yield run


@pytest.fixture(scope='module')
def recorded():
    return ms.load_fixture()


def _apply_one(oracle):
    return lambda fn, v: int(oracle.math_apply(fn, np.array([v], dtype=np.float32)).view(np.uint32)[0])


def test_helpers():
    "the block walk covers 0 .. 2^32 - 1 once; keys order like floats; ulp_err is the definition of test_fast_build_gpu._ulp_err"
    bl = list(ms.blocks())
    assert len(bl) == ms.N_BLOCKS and bl[0] == (0, 0) and bl[-1][1] + ms.BLOCK == 1 << 32 and all(s == k * ms.BLOCK for k, s in bl)
    assert 65535 * ms.BLOCK * ms.BLOCK < 1 << 63
    v = np.array([-np.inf, -3.0, -1e-45, 0.0, 1e-45, 1.0, 88.72, np.inf], dtype=np.float32)
    ks = [ms.K(x) for x in v]
    assert ks == sorted(ks) and ms.K(-0.0) == 0 and ms.key_of(0xffffffff) < -ms.INF_BITS and ms.key_of(0x7fc00000) > ms.INF_BITS
    rng = np.random.RandomState(1)
    want = np.concatenate([np.exp(rng.uniform(-104, 88, 1000)), [0.0, 1e-45, 1.0, 2.0 ** -126]])
    got = (want * (1 + rng.uniform(-2e-7, 2e-7, want.size))).astype(np.float32)
    w32 = want.astype(np.float32)
    old = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(np.spacing(w32)).astype(np.float64), 1.4012984643e-45)
    np.testing.assert_array_equal(ms.ulp_err(got, want), old)
    import torch
    np.testing.assert_array_equal(ms.ulp_err_torch(torch.from_numpy(got), torch.from_numpy(want)).numpy(), old)
    y = np.array([np.nan, -np.nan, 0.0, -0.0, 1.0], dtype=np.float32)
    np.testing.assert_array_equal(OPS.out_bits(y), [ms.NAN_BITS, ms.NAN_BITS, 0, 0x80000000, 0x3f800000])
    np.testing.assert_array_equal(ms.TorchOps(torch.device('cpu')).out_bits(torch.from_numpy(y)).numpy(), OPS.out_bits(y))


@pytest.mark.parametrize('probe', ms.PROBES)
def test_recorded_checksums_are_the_live_oracle(apply, pool, recorded, probe):
    "a changed header changes the oracle: then tools/math_checksums.py has to run again"
    w = OPS.weights()
    got = list(pool.map(lambda k: ms.checksum(OPS, apply(probe, OPS.as_float(OPS.input_bits(k * ms.BLOCK, ms.BLOCK))), w)[0], SAMPLE))
    want = recorded[ms.PROBES.index(probe)]
    for k, row in zip(SAMPLE, got):
        assert [int(v) for v in row] == [int(v) for v in want[k]], 'block %d (from 0x%08x) of %s' % (k, k * ms.BLOCK, probe)


def test_checksum_is_the_same_in_torch(oracle):
    "the device side of the comparison computes the sums with torch"
    import torch
    y = oracle.math_apply('log', OPS.as_float(OPS.input_bits(0x7f800000 - 2 * ms.BLOCK, 4 * ms.BLOCK)))           # finite, +inf and NaN inputs
    t = ms.checksum(ms.TorchOps(torch.device('cpu')), torch.from_numpy(y)).numpy()
    np.testing.assert_array_equal(t, ms.checksum(OPS, y))
    assert t.shape == (4, 3) and int(t.max()) < 1 << 61


@pytest.mark.parametrize('fn', ms.ACCURACY_FUNCTIONS)
def test_oracle_accuracy_against_float64(oracle, apply, pool, fn):
    """the statements of the GPU sweep, on the sample blocks and on the blocks of the recorded worst cases; each recorded worst case is
    reproduced, and nothing on these blocks is worse"""
    worst = {key[1:]: v for key, v in ms.ORACLE_WORST.items() if key[0] == fn}
    ks = sorted(set(SAMPLE) | set(ms.block_of(x) for x, _ in worst.values()))

    def one(k):
        t = ms.Tally(fn, _apply_one(oracle))
        t.add(OPS, k * ms.BLOCK, apply(fn, OPS.as_float(OPS.input_bits(k * ms.BLOCK, ms.BLOCK))))
        return t
    tallies = list(pool.map(one, ks))
    for t in tallies:
        t.check()
    for key, (xb, err) in worst.items():
        e, at, _ = max((t.worst[key] for t in tallies), key=lambda v: v[0])
        assert ms.same_input(fn, at, xb) and ms.same_figure(e, err), (fn, key, hex(at), e, hex(xb), err)


@pytest.mark.parametrize('relation', ms.LEAN_FORMS, ids=[r[0] + '-' + r[1] for r in ms.LEAN_FORMS])
def test_lean_forms_equal_the_general_forms(apply, pool, relation):
    for cnt, xb, a, g in pool.map(lambda k: ms.lean_mismatches(OPS, apply, relation, k * ms.BLOCK, ms.BLOCK), SAMPLE):
        assert cnt == 0, '%s(0x%08x) = 0x%08x, %s gives 0x%08x; %d such inputs in the block' % (relation[0], xb, a, relation[1], g, cnt)


@pytest.mark.parametrize('fn', ['tanh', 'tanh_abs'])
def test_tanh_forms_are_odd(apply, pool, fn):
    "f(-x) is f(x) with the sign bit flipped, zero results included (torch.tanh(-0.0) is -0.0)"
    for cnt, xb, p, m in pool.map(lambda k: ms.odd_mismatches(OPS, apply, fn, k * ms.BLOCK, ms.BLOCK), [k for k in SAMPLE if k < ms.N_BLOCKS // 2]):
        assert cnt == 0, '%s(0x%08x) = 0x%08x but %s(0x%08x) = 0x%08x; %d such inputs in the block' % (fn, xb, p, fn, xb | 1 << 31, m, cnt)
