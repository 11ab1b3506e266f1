"""Deterministic structured instance families for the test-suite (a plain module like helpers.py).

The uniform k-SAT batches of helpers.random_batch vary neither the clause length (1 to 5), nor the variable degree (Poisson around 10 to
13) nor the edges per variable (9 or more), and the kernels branch on exactly those quantities.  Every family here is a function
``(rng, ...) -> (n, clause_list)``; a batch holds 4 to 64 instances of ONE family (a NaN poison is batch-wide in the reference's semantics,
a single-instance batch takes the exact route, and batches of this size never fail their speculation) and goes through
dataset.instance_from_clauses / collate_segment exactly as helpers.random_batch does.

BATCHES maps a batch name to (builder, promise): ``instances(name)`` returns the list of (n, clause_list), ``batch(name)`` the collated
numpy batch, ``table(batch)`` the per-instance structure table the promises are asserted against (tests/test_families_host.py).
"""
import numpy as np

import helpers  # noqa: F401  (sys.path)
from pdp import generator
from pdp.factorgraph import dataset


# ---- the families -------------------------------------------------------------------------------------------------------------------
def _signs(rng, k):
    return rng.randint(0, 2, size=k) * 2 - 1


def hub(rng, d, n=60, m=None):
    "uniform 3-SAT plus d more 3-clauses through variable 1: its degree is d + (what the uniform part gives it)"
    m = int(rng.randint(150, 201)) if m is None else m
    clauses = generator.uniform_ksat(n, m, 3, rng)
    for _ in range(d):
        others = rng.choice(n - 1, size=2, replace=False) + 2
        sg = _signs(rng, 3)
        clauses.append([int(sg[0])] + [int(v * s) for v, s in zip(others, sg[1:])])
    return n, clauses


def sparse_hub(rng, d, n):
    "a hub of d more 3-clauses through variable 1 of a sparse regular (4, 3) instance: a long row where the solver re-reads its work items"
    n, clauses = regular(rng, 4, 3, n)
    for _ in range(d):
        others = rng.choice(n - 1, size=2, replace=False) + 2
        sg = _signs(rng, 3)
        clauses.append([int(sg[0])] + [int(v * s) for v, s in zip(others, sg[1:])])
    return n, clauses


def long_clause(rng, k, at, n=300, m=1100):
    "uniform 3-SAT with ONE clause of k literals at clause position `at` (negative: from the end)"
    clauses = generator.uniform_ksat(n, m - 1, 3, rng)
    vs = rng.choice(n, size=k, replace=False) + 1
    clauses.insert(at if at >= 0 else m + at, [int(v * s) for v, s in zip(vs, _signs(rng, k))])
    return n, clauses


def only_long(rng, k, n, m):
    "every clause has k literals"
    return n, generator.uniform_ksat(n, m, k, rng)


def regular(rng, d, k, n):
    """sparse and peel-resistant: every variable occurs exactly d times with alternating signs (no pure literal), the occurrences are
    shuffled and cut into k-tuples, and a tuple with a repeated variable is dropped (so a few variables occur less often)"""
    occ = np.repeat(np.arange(1, n + 1), d) * np.tile(np.array([1, -1])[np.arange(d) % 2], n)
    occ = occ[rng.permutation(occ.size)]
    clauses = []
    for i in range(0, occ.size - k + 1, k):
        c = [int(x) for x in occ[i:i + k]]
        if len({abs(x) for x in c}) == k:
            clauses.append(c)
    return n, clauses


def power_law(rng, beta, n, alpha=3.5):
    "3-SAT with m = alpha n whose variable i is drawn with weight i^-beta"
    w = np.arange(1, n + 1, dtype=np.float64) ** -beta
    w /= w.sum()
    clauses = []
    for _ in range(int(alpha * n)):
        vs = rng.choice(n, size=3, replace=False, p=w) + 1
        clauses.append([int(v * s) for v, s in zip(vs, _signs(rng, 3))])
    return n, clauses


def community(rng, variable):
    """the package's own Community Attachment generators (pdp.cnf_generators), which draw from numpy's global generator: seeded from
    `rng` and restored afterwards"""
    from pdp.cnf_generators import ModularCNFGenerator, VariableModularCNFGenerator
    saved = np.random.get_state()
    np.random.seed(int(rng.randint(1 << 30)))
    try:
        if variable:
            g = VariableModularCNFGenerator(2, 8, 60, 200, 0.3, 0.9, 4, 12, 3.0, 5.0)
        else:
            g = ModularCNFGenerator(3, 60, 200, 0.3, 0.9, 4, 12, 3.0, 4.2)
        n, m, gm, ef = g.generate()[:4]
    finally:
        np.random.set_state(saved)
    clauses = [[] for _ in range(m)]
    for v, c, s in zip(gm[0], gm[1], ef):
        clauses[int(c)].append(int((v + 1) * s))
    return n, clauses


def ladder(rng, n, alpha):
    return n, generator.uniform_ksat(n, int(round(alpha * n)), 3, rng)


def unit_chain(L):
    "[[1], [-1, 2], [-2, 3], ...]: simplify fixes one variable per fix-point round"
    return L, [[1]] + [[-i, i + 1] for i in range(1, L)]


def pure_cascade(L):
    "[[1, 2], [-2, -3], [3, 4], ...]: variable 1 is pure, and removing its clause makes the next variable pure, L times"
    return L + 1, [[i, i + 1] if i % 2 else [-i, -(i + 1)] for i in range(1, L + 1)]


def minimal(rng):
    "the smallest shapes, one batch"
    same = [2, -3, 5]
    return [(1, [[1]]),
            (1, [[-1]] * 40),
            (2, [[1, -2]]),
            (2, [[1, 2], [-1, 2], [1, -2], [-1, -2]]),
            (5, [list(same) for _ in range(12)]),
            (20, [[int(v) for v in rng.choice(20, size=3, replace=False) + 1] for _ in range(50)]),
            (20, [[-int(v) for v in rng.choice(20, size=3, replace=False) + 1] for _ in range(50)])]


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
LONG_AT = (0, 5, 63, 64, 255, 256, -1)
LADDER_42 = list(range(100, 701, 20))
LADDER_30 = list(range(100, 601, 20))


def _windows(sizes, width=5):
    "overlapping windows: every pair of neighbouring sizes shares a batch, so each routing limit is crossed inside one"
    out = []
    i = 0
    while i + width < len(sizes):
        out.append(sizes[i:i + width])
        i += width - 1
    return out + [sizes[-width:]]


def _each(fn, args, seed):
    return lambda: [fn(np.random.RandomState(seed + i), *a) for i, a in enumerate(args)]


BATCHES = {}
# promise keys: deg = (lo, hi) bounds of the batch's maximum variable degree, k = maximum clause length (exact), epv = (lo, hi) bounds of
# edges per variable over the batch, nan1 = the oracle's first sweep poisons the batch (exempt from the float comparison of pdp_sp_solve)


def _add(name, builder, **promise):
    assert name not in BATCHES
    BATCHES[name] = (builder, promise)


for ds in ((15, 16, 17), (31, 32, 33), (64,), (128,), (254, 255, 256, 257), (1000,)):
    _add('hub-' + '-'.join(str(d) for d in ds), _each(hub, [(d,) for d in ds for _ in range(-(-4 // len(ds)))], 1000 + ds[0]),
         deg=(max(ds), max(ds) + 30), k=3, nan1=ds[0] >= 1000)
_add('hub-3000', _each(hub, [(64,), (3000, 200, 600), (64,), (128,)], 4000), deg=(3000, 3030), k=3, nan1=True, mixed_routes=True)
_add('sparsehub-300', _each(sparse_hub, [(300, 600)] * 4, 4100), deg=(300, 310), k=3)
for k_ in (63, 64, 65, 255, 256, 257):
    _add('long-%d' % k_, _each(long_clause, [(k_, at) for at in LONG_AT], 5000 + k_), k=k_, deg=(15, 45))
_add('long-only-10', _each(only_long, [(10, 60, 240)] * 4, 6000), k=10, epv=(39, 41))
_add('long-only-100', _each(only_long, [(100, 300, 40)] * 4, 6100), k=100, epv=(13, 14))
_add('long-1000', _each(long_clause, [(1000, at, 1200, 4400) for at in (0, 64, 255, -1)], 6200), k=1000, deg=(15, 45), hbm_all=True)
for n_ in (130, 200, 250):
    _add('regular-4-2-n%d' % n_, _each(regular, [(4, 2, n_)] * 4, 7000 + n_), deg=(4, 4), k=2, epv=(3.5, 4.0))
for n_ in (300, 600, 900, 1000):
    _add('regular-4-3-n%d' % n_, _each(regular, [(4, 3, n_)] * 4, 7100 + n_), deg=(4, 4), k=3, epv=(3.5, 4.0))
for n_ in (500, 700, 800):
    _add('regular-6-3-n%d' % n_, _each(regular, [(6, 3, n_)] * 4, 7200 + n_), deg=(6, 6), k=3, epv=(5.5, 6.0), hbm_all=n_ == 800)
_add('power-0.5', _each(power_law, [(0.5, n_) for n_ in (50, 100, 150, 200, 250, 300)], 8000), k=3, deg=(20, 120))
_add('power-0.9', _each(power_law, [(0.9, n_) for n_ in (50, 100, 150, 200, 250, 300)], 8100), k=3, deg=(80, 480), nan1=True)     # (variable 1 of n = 300 expects 3 m / sum(i^-0.9) = 380 occurrences)
_add('community-modular', _each(community, [(False,)] * 8, 9000), k=3)
_add('community-variable', _each(community, [(True,)] * 8, 9100), k=8)
for i_, w_ in enumerate(_windows(LADDER_42)):
    _add('ladder-4.2-n%d-%d' % (w_[0], w_[-1]), _each(ladder, [(n_, 4.2) for n_ in w_], 10000 + 10 * i_), k=3, epv=(12.5, 12.61))
for i_, w_ in enumerate(_windows(LADDER_30)):
    _add('ladder-3.0-n%d-%d' % (w_[0], w_[-1]), _each(ladder, [(n_, 3.0) for n_ in w_], 11000 + 10 * i_), k=3, epv=(8.95, 9.01))
for L_ in (100, 1000, 4000):
    _add('chains-%d' % L_, (lambda L: lambda: [unit_chain(L), ladder(np.random.RandomState(12000 + L), 60, 4.0), pure_cascade(L), unit_chain(L // 2 + 1)])(L_),
         k=3, deg=(2, 40))
_add('minimal', lambda: minimal(np.random.RandomState(13000)), k=3)

NAMES = list(BATCHES)
# batches whose oracle run is NaN-poisoned in the first sweep: pdp_sp_solve's float comparison cannot go beyond the NaN pattern there, and
# the single-sweep and integer-state operators cover them instead
POISONED_IN_SWEEP_1 = [nm for nm in NAMES if BATCHES[nm][1].get('nan1')]
# batches that the oracle solves within three sweeps (any assignment satisfies clauses of 10 or 100 literals at a density an LDS image can
# hold; an unsatisfiable 10-SAT core needs 1 024 clauses): pdp_sp_solve is compared on the sweeps that run, and the row kernels cover the rest
SOLVED_AT_ONCE = ['long-only-10', 'long-only-100']
# batches that the long-running candidates live in (their own pytest ids, so that a time limit names them)
LONG_RUNNING = ['chains-4000', 'long-1000']


def promise(name):
    return BATCHES[name][1]


def anchored(inst):
    """The first instance of a batch gets one more variable under a unit clause at its end.  simplify() fixes it, and an inactive variable is
    the exact zero the persistent solver's speculation counts on in every batch-wide minimum: without one in the batch (a hub or regular
    batch has no pure literal and no unit clause) the LDS-resident run is rolled back and the lock-step launch serves the call -- and the
    kernel under test would never be compared."""
    (n, clauses), rest = inst[0], inst[1:]
    return [(n + 1, clauses + [[n + 1]])] + rest


def instances(name):
    inst = BATCHES[name][0]()
    return inst if name.startswith(('chains', 'minimal')) else anchored(inst)


def collate(inst, prefix='f'):
    return dataset.collate_segment([dataset.instance_from_clauses(n, c, label=-1, name='%s%d' % (prefix, i)) for i, (n, c) in enumerate(inst)])


def batch(name):
    return collate(instances(name), name)


def table(b):
    "per instance: variables, clauses, edges, maximum degree, maximum clause length -- computed from the collated batch"
    gm, bvm, bfm = b['graph_map'], b['batch_variable_map'], b['batch_function_map']
    deg = np.bincount(gm[0], minlength=bvm.size)
    length = np.bincount(gm[1], minlength=bfm.size)
    B = int(bvm.max()) + 1
    rows = []
    for i in range(B):
        vs, fs = bvm == i, bfm == i
        rows.append(dict(n=int(vs.sum()), m=int(fs.sum()), e=int(length[fs].sum()), max_degree=int(deg[vs].max()), max_length=int(length[fs].max())))
    return rows


def lds_image_bytes(n, m, e):
    "size of an instance's image in the LDS-resident solver (lds2_bytes_for of csrc/pdp_solve.hip); an instance fits up to 159 KiB"
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    return 5 * a16(4 * e) + 3 * a16(2 * e) + a16(2 * (n + 1)) + a16(2 * (m + 1)) + a16(4 * (m + 8)) + a16(4 * m) + 7 * a16(4 * n) + a16(n) + a16(2 * n)


def fits_lds(row):
    return lds_image_bytes(row['n'], row['m'], row['e']) <= 159 * 1024 and row['e'] < 65535 and row['n'] < 16384 and row['m'] < 16384


def solver_launch(rows, threads=None):
    """the launch pdp_sp_solve gives the LDS-resident solver for a batch (the rules of pdp_sp_solve / k_sp_solve_lds in csrc/pdp_solve.hip):
    threads per workgroup -- 256 up to 1 024 edges, 512 while the largest fitting image is within 80 KiB, else 1 024 -- and per fitting
    instance whether the P4 work item is cached in registers (2 n <= threads) and how many helper waves take the clause rows"""
    fit = [r for r in rows if fits_lds(r)]
    if not fit:
        return None
    image = lds_image_bytes(max(r['n'] for r in fit), max(r['m'] for r in fit), max(r['e'] for r in fit))
    nt = threads or (256 if max(r['e'] for r in fit) <= 1024 else (1024 if image > 80 * 1024 else 512))
    nw = nt // 64
    return dict(threads=nt, image=image, cached=[2 * r['n'] <= nt for r in fit], helpers=[nw - min((r['n'] + 63) // 64, nw) for r in fit])


def walksat_lds_bytes(n, m, e):
    "image of an instance in the LDS-resident Walk-SAT kernel (ws_lds_bytes of csrc/pdp_walksat.hip); an instance fits up to 64 KiB"
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    return 3 * a16(2 * e) + a16(2 * (n + 1)) + a16(2 * (m + 1)) + 4 * a16(4 * n) + 3 * a16(4 * m) + a16(m)


def simplify_lds_bytes(n, m, e):
    "image of the LDS-resident simplify (simplify_lds_bytes of csrc/pdp_solve.hip), sized by the batch's largest n, m, e; up to 64 KiB"
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    return 3 * a16(2 * e) + a16(2 * (n + 1)) + a16(2 * (m + 1)) + 5 * a16(4 * n) + a16(4 * m) + a16(n) + 2 * a16(m)


def first_nan_sweep(res):
    "index of the first sweep of an oracle forward(trace_float=True) whose surveys hold a NaN, or None"
    for s in range(res['iterations_run']):
        if np.isnan(res['trace_q'][s]).any() or np.isnan(res['trace_fs'][s]).any():
            return s
    return None


def sweep_plan(forward, T=40):
    """The compared runs of pdp_sp_solve on one batch: ``forward(T)`` is an oracle forward with trace_float=True on a fresh problem.
    Returns the list of sweep counts: T itself, and -- where the oracle poisons the batch before T -- also the last NaN-free sweep count
    (the poisoned run is kept: its NaN pattern and the integer state behind it must match too)."""
    s = first_nan_sweep(forward(T))
    return [T] if s is None or s == 0 else [T, s]


# ---- instances for the complete solver ------------------------------------------------------------------------------------------------
def exact_cases():
    "family instances small enough for the reference DPLL of test_exact_host.py: list of (name, n, clause_list)"
    out = []
    R = np.random.RandomState
    for i, d in enumerate((15, 16, 17, 31, 32, 33, 64)):
        out.append(('hub-%d' % d,) + hub(R(20000 + i), d, n=24, m=96))
    for i, (k, at) in enumerate(((20, 0), (20, 63), (20, 64), (30, -1), (30, 5), (12, 100))):
        out.append(('long-%d@%d' % (k, at),) + long_clause(R(20100 + i), k, at, n=40, m=172))
    for i, (d, k, n) in enumerate(((4, 2, 40), (4, 3, 45), (6, 3, 40), (6, 2, 30), (8, 3, 30), (8, 2, 24))):
        out.append(('regular-%d-%d-n%d' % (d, k, n),) + regular(R(20200 + i), d, k, n))
    for i, beta in enumerate((0.5, 0.5, 0.9, 0.9, 0.9, 0.5)):
        out.append(('power-%g-%d' % (beta, i),) + power_law(R(20300 + i), beta, 40, alpha=4.3))
    for i, (n, c) in enumerate(minimal(R(13000))):
        out.append(('minimal-%d' % i, n, c))
    for i, n in enumerate((20, 20, 40, 40, 40, 60, 60, 60, 60, 60)):
        out.append(('ladder-n%d-%d' % (n, i),) + ladder(R(20400 + i), n, 4.26))
    return out


def threshold_cores(count=4, n=50):
    "threshold 3-SAT instances on n variables (alpha 4.26), the hard cores of the composed instances: both answers occur among them"
    return [ladder(np.random.RandomState(20500 + i), n, 4.26) for i in range(count)]


def compose(core, big, place):
    """disjoint union of a small core and a big instance on their own variables: the core's variables and clauses `first`, `last` or
    `interleaved` (evenly spread over the variable ids and the clause positions).  Returns (n, clause_list, core_variables)."""
    (nc, cc), (nb, cb) = core, big
    n = nc + nb
    if place == 'first':
        core_ids = np.arange(1, nc + 1)
    elif place == 'last':
        core_ids = np.arange(nb + 1, n + 1)
    else:
        core_ids = 1 + (np.arange(nc) * n) // nc
    is_core = np.zeros(n + 1, bool)
    is_core[core_ids] = True
    big_ids = np.nonzero(~is_core[1:])[0] + 1
    ren = lambda c, ids: [int(ids[abs(l) - 1]) * (1 if l > 0 else -1) for l in c]  # noqa: E731
    cc2, cb2 = [ren(c, core_ids) for c in cc], [ren(c, big_ids) for c in cb]
    if place == 'first':
        clauses = cc2 + cb2
    elif place == 'last':
        clauses = cb2 + cc2
    else:
        clauses, step, j = [], max(1, len(cb2) // max(1, len(cc2))), 0
        for i, c in enumerate(cb2):
            if i % step == 0 and j < len(cc2):
                clauses.append(cc2[j]); j += 1
            clauses.append(c)
        clauses += cc2[j:]
    return n, clauses, core_ids


# ---- instances wider than one wave for the complete solvers ------------------------------------------------------------------------
def fan(n, seed, F=100):
    """threshold 3-SAT (alpha 4.26, three distinct variables per clause) on variables 1 .. n behind a unit clause on variable a = n + 1
    and F implications a -> a + i: one pass at level 0 assigns F variables, and every later trail is longer than F"""
    rng = np.random.RandomState(seed)
    a = n + 1
    clauses = [[a]] + [[-a, a + i] for i in range(1, F + 1)]
    for _ in range(int(round(4.26 * n))):
        vs = rng.choice(n, size=3, replace=False) + 1
        clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
    return n + 1 + F, clauses


def wide(D):
    """a_j = j, b_j = D + j, z = 2 D + 1, w = 2 D + 2: D binary clauses [a_j, b_j], then the four sign patterns of z and w behind all the
    -a_j.  Satisfiable (some a_j false); the searches first make every a_j true and meet conflict, reason and learned clauses of D + 1
    and D + 2 literals"""
    z, w = 2 * D + 1, 2 * D + 2
    no_a = [-j for j in range(1, D + 1)]
    return 2 * D + 2, [[j, D + j] for j in range(1, D + 1)] + [no_a + [sz * z, sw * w] for sz in (1, -1) for sw in (1, -1)]


def stride(inst, s):
    "variable v becomes 1 + (v - 1) s: a monotone renumbering (the searches take the same steps) that spreads the ids in use over s times as many"
    n, clauses = inst
    return 1 + (n - 1) * s, [[(1 + (abs(l) - 1) * s) * (1 if l > 0 else -1) for l in c] for c in clauses]


def wide_kept(D):
    """wide(D) plus a second z / w gadget (z2 = 2 D + 3, w2 = 2 D + 4) behind -a_1 .. -a_{D-1} and -b_D, which opens only after the first
    gadget has made a_D false by a learned clause of D literals.  At an arena of 3 D + 4 words the clause the second gadget learns does
    not fit: the reduction keeps that D-literal reason, moves it to the front, and the next analysis resolves with it"""
    n, clauses = wide(D)
    z, w = n + 1, n + 2
    rest = [-j for j in range(1, D)] + [-2 * D]
    return n + 2, clauses + [rest + [sz * z, sw * w] for sz in (1, -1) for sw in (1, -1)]


def far_uip(K):
    """d = 1 decides true (K + 1 occurrences of each sign) and one pass assigns c = 2 and f_1 .. f_K = 3 .. K + 2 in this order; c implies
    x and y, which contradict each other.  The analysis resolves on y and x and then walks back over the K entries f_K .. f_1 to reach c,
    its first UIP; chronological backtracking undoes K + 4 entries in one step"""
    x, y, g = K + 3, K + 4, K + 5
    clauses = [[-1, 2]] + [[-1, 2 + i] for i in range(1, K + 1)] + [[1, g + i] for i in range(K + 1)]
    return g + K, clauses + [[-2, x], [-2, y], [-x, -y]]
