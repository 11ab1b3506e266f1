"""Rates of the batched complete solver (pdp_exact_solve): per row, the kernel time from device events (the second call on the problem:
the one-time routing preparation is not in it), instances per second, SAT / UNSAT / undecided counts, median / p99 / max work
(clause-literal reads per instance), literal reads per second, and the wall time of labelling the batch from loader items (collate,
problem set-up, the first call with its preparation, results back on the host).
Usage: python tools/exact_time.py [row ...]   (rows a b c d e; default all)"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
from pdp import native  # noqa: E402
from pdp.cnf_generators import UniformCNFGenerator  # noqa: E402
from pdp.factorgraph import dataset  # noqa: E402


def planted_item(n, alpha, seed):
    "3-SAT with a planted solution (x = RandomState(seed) bits): every clause keeps a literal true under it"
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 2, size=n)
    m, rows = int(round(alpha * n)), []
    while sum(len(r) for r in rows) < m:
        vs = rng.randint(0, n, size=(2 * m, 3))
        sg = rng.choice([-1, 1], size=(2 * m, 3))
        srt = np.sort(vs, axis=1)
        rows.append(((vs + 1) * sg)[(srt[:, 1:] != srt[:, :-1]).all(axis=1) & ((x[vs] == 1) == (sg > 0)).any(axis=1)])
    lits = np.concatenate(rows)[:m]
    gm = np.stack((np.abs(lits).reshape(-1) - 1, np.repeat(np.arange(m), 3))).astype(np.int32)
    return n, m, gm, np.sign(lits).reshape(-1).astype(np.float32), 1.0, ['planted_%d' % n]


def gcnf_items(B):
    np.random.seed(0)
    g = UniformCNFGenerator(4, 100, 2, 10, 2, 10)
    out = []
    for i in range(B):
        n, m, gm, ef, _, _, _ = g.generate()
        out.append((n, m, gm.astype(np.int32), ef.astype(np.float32), -1.0, ['gcnf_%d' % i]))
    return out


ROWS = {
    'a': ('uniform 3-SAT n=100 m=426, B=5000', lambda: dataset.random_ksat_items(5000, 100, 3, m=426, seed=0)),
    'b': ('uniform 3-SAT n=150 m=639, B=2000', lambda: dataset.random_ksat_items(2000, 150, 3, m=639, seed=0)),
    'c': ('uniform 3-SAT n=200 m=852, B=1000', lambda: dataset.random_ksat_items(1000, 200, 3, m=852, seed=0)),
    'd': ('gcnf mix UniformCNFGenerator(4,100,2,10,2,10), B=5000', lambda: gcnf_items(5000)),
    'e': ('row (a) + one planted 3-SAT n=20000 alpha=2 (HBM route), B=5001',
          lambda: dataset.random_ksat_items(2500, 100, 3, m=426, seed=0) + [planted_item(20000, 2.0, 7)]
          + dataset.random_ksat_items(2500, 100, 3, m=426, seed=2500)),
}


def run(key):
    title, make = ROWS[key]
    items = make()
    dev = torch.device('cuda:0')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = dataset.to_torch(dataset.collate_segment(items), dev)
    p = native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(items))
    st, _, wk = p.exact_solve()
    status, work = st.cpu().numpy(), wk.cpu().numpy()
    wall = time.perf_counter() - t0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    st2, _, wk2 = p.exact_solve()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1])
    assert np.array_equal(st2.cpu().numpy(), status) and np.array_equal(wk2.cpu().numpy(), work), "second call differs"
    B = len(items)
    sat, unsat, und = int((status == 1).sum()), int((status == 0).sum()), int((status == -1).sum())
    print("(%s) %s: E=%d  kernel %.2f ms  %.0f instances/s  SAT %d  UNSAT %d  undecided %d  work median %d  p99 %d  max %d  "
          "%.3g literal reads/s  labelling wall %.3f s (set-up included)"
          % (key, title, p.E, ms, B / (ms * 1e-3), sat, unsat, und, int(np.median(work)), int(np.percentile(work, 99)), int(work.max()),
             float(work.sum()) / (ms * 1e-3), wall), flush=True)
    if key == 'e':
        big = next(i for i, it in enumerate(items) if it[5] and it[5][0].startswith('planted'))
        print("    planted n=20000 instance: status %d  work %d" % (int(status[big]), int(work[big])), flush=True)


if __name__ == '__main__':
    native.require_gpu()
    for k in (sys.argv[1:] or sorted(ROWS)):
        run(k)
