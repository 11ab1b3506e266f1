"""Runs the CPU oracle (oracle/libpdp_oracle.so: include/pdp_math.h compiled for the host) over all 2^32 float32 inputs of every
single-argument math probe.

python tools/math_checksums.py [--out FILE]
    writes the per-block checksums (tests/math_sweep.py: checksum) to tests/golden/math_checksums.npz: `sums` uint64
    [probes, 2^32 / BLOCK, 3], `probes`, `block`.  tests/test_math_sweep_gpu.py compares every block of the device's outputs with
    it.  The file's bytes depend on the oracle's results only: run it again after a change of the header, and the diff says whether
    any output bit moved.  A few minutes on 8 cores.

python tools/math_checksums.py --accuracy [function ...]
    the same sweep against numpy float64 (tests/math_sweep.py: statements): prints, per statement, the worst input and its error, or
    how many inputs break it.  These are the figures in the comments of include/pdp_math.h, in DESIGN.md and in
    math_sweep.ORACLE_WORST.  About a minute per function on 8 cores.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'tests'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import math_sweep as ms  # noqa: E402
from oracle import binding  # noqa: E402

OPS = ms.NumpyOps()


def oracle_block(probe, start, n=ms.BLOCK):
    return binding.math_apply(probe, OPS.as_float(OPS.input_bits(start, n)))


def oracle_one(probe, value):
    return int(binding.math_apply(probe, np.array([value], dtype=np.float32)).view(np.uint32)[0])


def pool():
    return ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))          # ctypes and numpy's loops release the GIL


def checksums():
    w = OPS.weights()
    sums = np.zeros((len(ms.PROBES), ms.N_BLOCKS, 3), dtype=np.uint64)
    with pool() as ex:
        for p, probe in enumerate(ms.PROBES):
            t0 = time.time()
            rows = ex.map(lambda kb: ms.checksum(OPS, oracle_block(probe, kb[1]), w)[0], ms.blocks())
            for k, row in enumerate(rows):
                sums[p, k] = row.astype(np.uint64)
            print('%-20s %6.1f s' % (probe, time.time() - t0), flush=True)
    return sums


def accuracy(fn):
    def one(kb):
        t = ms.Tally(fn, oracle_one)
        t.add(OPS, kb[1], oracle_block(fn, kb[1]))
        return t
    total = ms.Tally(fn, oracle_one)
    with pool() as ex:
        for t in ex.map(one, ms.blocks()):                                         # in block order: of equal errors the first input stays
            for key, v in t.worst.items():
                if key not in total.worst or v[0] > total.worst[key][0]:
                    total.worst[key] = v
            for name, (c, x0, y0) in t.broken.items():
                c0, x1, y1 = total.broken.get(name, (0, x0, y0))
                total.broken[name] = (c0 + c, x1, y1)
            total.seen += t.seen
    assert total.seen == 1 << 32
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=ms.GOLDEN_FILE)
    ap.add_argument('--accuracy', nargs='*', default=None, metavar='FUNCTION', help='of ' + ' '.join(ms.ACCURACY_FUNCTIONS))
    a = ap.parse_args()
    binding.build()
    if a.accuracy is not None:
        for fn in a.accuracy or ms.ACCURACY_FUNCTIONS:
            t0 = time.time()
            t = accuracy(fn)
            print('\n'.join(t.report()), flush=True)
            print('%-10s %.1f s' % (fn, time.time() - t0), flush=True)
        return
    ms.save_fixture(a.out, checksums())
    print('wrote %s (%d bytes)' % (a.out, os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
