"""The backward check of a proof of unsatisfiability (pdp_exact_trim, include/pdp_hip.h) stated in plain Python: which original clauses
(the core) and which lemmas the refutation actually rests on.  It shares no code with the searches; of the forward checker
(tests/exact_proof_model.py) it reuses ``_scan`` only, so work counts the same clause-literal reads as the GPU and all outputs can be
compared with array_equal."""
import functools

import numpy as np

from exact_proof_model import _scan


def trim(n, clauses, region_words, proof_len, budget=0, stats=None):
    """(verdict 1 / 0 / -1, fail_at, work, core, keep_lemmas) of one instance that was answered "unsatisfiable".  ``region_words``: the
    whole region of the instance (int32 words, any content); ``proof_len``: the words of it that are said to hold lemmas.  core: one
    0/1 per clause; keep_lemmas: one 0/1 per lemma of the first proof_len words (None when they do not parse or the instance is not
    judged).  ``stats``: a dict that counts the branches taken."""
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in clauses for l in c])
    m = len(clauses)
    if budget <= 0:
        budget = 1 << 32
    stats = {} if stats is None else stats

    def count(key):
        stats[key] = stats.get(key, 0) + 1

    def peak(key, x):
        stats[key] = max(stats.get(key, 0), x)

    nothing = [0] * m
    if proof_len < 0 or proof_len > len(region_words):
        return -1, -1, 0, nothing, None
    orig = [[((abs(l) - 1) << 1) | (1 if l < 0 else 0) for l in c] for c in clauses]
    # step 1: every lemma is validated before any is used
    w = [int(x) for x in region_words[:proof_len]]
    lemmas, pos = [], 0
    while pos < proof_len:
        ln = w[pos]
        if ln < 0 or pos + 1 + ln > proof_len:
            return 0, len(lemmas), 0, nothing, None
        lits = w[pos + 1:pos + 1 + ln]
        if any(L < 0 or (L >> 1) >= n for L in lits):
            return 0, len(lemmas), 0, nothing, None
        lemmas.append(lits)
        pos += 1 + ln
    L = len(lemmas)
    peak('peak-lemmas', L)
    every = orig + lemmas                                                           # lemma j is clause m + j
    marked = [False] * L + [True]
    core = [0] * m
    none = [0] * L
    work = 0
    # step 2: from the empty clause backwards, only what is needed
    for i in range(L, -1, -1):
        if not marked[i]:
            count('skipped')
            continue
        lits = lemmas[i] if i < L else []
        peak('peak-checked-lemma', len(lits))
        val = [0] * n
        work += len(lits)
        # A marked lemma was falsified or unit in some pass, so it does not hold both polarities of a variable (such a lemma always has a
        # true literal or two different unassigned ones): the forward checker's "accepted at once" has no counterpart here.
        for lit in lits:
            assert val[lit >> 1] in (0, 2 - (lit & 1))
            val[lit >> 1] = 2 - (lit & 1)                                           # the value that makes the literal false
        rsn = {}
        while True:
            if work >= budget:
                return -1, -1, work, nothing, none
            confl, req = None, {}
            for ci in range(m + i):
                reads, kind, lit = _scan(every[ci], val)
                work += reads
                if kind == 'conflict':
                    if confl is None:
                        confl = ci
                elif kind == 'unit':
                    req.setdefault(lit, ci)
            if confl is not None:
                count('start-falsified')
                start = [confl]
                break
            both = sorted(lit >> 1 for lit in req if lit & 1 and lit ^ 1 in req)
            if both:
                count('start-both')
                start = [req[both[0] << 1], req[(both[0] << 1) | 1]]
                break
            if not req:
                return 0, i, work, nothing, none
            peak('peak-batch', len(req))
            for lit, ci in req.items():
                val[lit >> 1] = 1 + (lit & 1)
                rsn[lit >> 1] = ci
        # the closure: the start set and, transitively, the reasons of the variables its clauses mention
        reached, todo = set(), list(start)
        while todo:
            ci = todo.pop()
            if ci in reached:
                continue
            reached.add(ci)
            work += len(every[ci])
            peak('peak-antecedent', len(every[ci]))
            for lit in every[ci]:
                if (lit >> 1) in rsn:
                    todo.append(rsn[lit >> 1])
        for ci in reached:
            if ci < m:
                core[ci] = 1
            else:
                marked[ci - m] = True
        count('closure-lemma' if any(ci >= m for ci in reached) else 'closure-originals')
    return 1, -1, work, core, [int(x) for x in marked[:L]]


def keep_words(region_words, proof_len, keep_lemmas):
    "keep_lemmas per proof word: 1 on the length word and the literals of a kept lemma, 0 on the other words among the first proof_len"
    out = np.zeros(max(int(proof_len), 0), dtype=np.int8)
    if keep_lemmas is None:
        return out
    pos = 0
    for k in keep_lemmas:
        ln = int(region_words[pos])
        out[pos:pos + 1 + ln] = k
        pos += 1 + ln
    return out


def trim_all(instances, status, regions, proof_len, budget=0, stats=None):
    """trim() over a list, as the entry point answers: (verdict int8 [N], fail_at int32 [N], work int64 [N], core lists, keep word arrays
    of proof_len words (None: the instance is not judged, nothing of its region is written), n_core int32 [N], n_keep int32 [N]).
    Only status 0 is judged."""
    verdict, fail_at, work, cores, keeps, n_core, n_keep = [], [], [], [], [], [], []
    for i, (n, c) in enumerate(instances):
        judged = int(status[i]) == 0 and 0 <= int(proof_len[i]) <= len(regions[i])
        r = trim(n, c, regions[i], int(proof_len[i]), budget, stats) if judged else (-1, -1, 0, [0] * len(c), None)
        verdict.append(r[0]); fail_at.append(r[1]); work.append(r[2]); cores.append(np.asarray(r[3], dtype=np.int8))
        keeps.append(keep_words(regions[i], proof_len[i], r[4]) if judged else None)
        n_core.append(int(sum(r[3]))); n_keep.append(int(sum(r[4])) if r[4] is not None else 0)
    return (np.array(verdict, dtype=np.int8), np.array(fail_at, dtype=np.int32), np.array(work, dtype=np.int64), cores, keeps,
            np.array(n_core, dtype=np.int32), np.array(n_keep, dtype=np.int32))


def core_instance(inst, core):
    "the sub-instance of the clauses with core = 1, over the same variables"
    n, clauses = inst
    return n, [c for c, k in zip(clauses, core) if k]


def kept(region_words, proof_len, keep_lemmas):
    "the kept lemmas, in order, as lists of literal codes"
    import exact_proof_model as pm
    return [x for x, k in zip(pm.parse(region_words[:proof_len]), keep_lemmas) if k]


# ---- the inputs shared by test_exact_trim_host.py and test_exact_trim_gpu.py: computed once per process, never modified by a test ------
@functools.lru_cache(maxsize=None)
def modular(count=8, n=60, alpha=4.0, seed=7):
    """community-attachment instances of ModularCNFGenerator(3, n, n, 0.8, 0.9, n // 10, n // 10, alpha, alpha + 0.4, 1) (pdp.cnf_generators,
    which draws from numpy's global generator: seeded and restored)"""
    from pdp.cnf_generators import ModularCNFGenerator
    saved = np.random.get_state()
    np.random.seed(seed)
    try:
        g = ModularCNFGenerator(3, n, n, 0.8, 0.9, n // 10, n // 10, alpha, alpha + 0.4, 1)
        out = []
        for _ in range(count):
            nn, m, gm, ef = g.generate()[:4]
            clauses = [[] for _ in range(m)]
            for v, c, s in zip(gm[0], gm[1], ef):
                clauses[int(c)].append((int(v) + 1) * (1 if s > 0 else -1))
            out.append((int(nn), clauses))
    finally:
        np.random.set_state(saved)
    return out


@functools.lru_cache(maxsize=None)
def base_cases():
    """The unsatisfiable runs of exact_proof_model.base_inputs() at arenas 0, 12 and 40: (instances, regions, proof_len, the trim_all of
    them, the branch statistics)."""
    import exact_proof_model as pm
    inst, runs = pm.base_inputs()
    batch, regions = [], []
    for A in (0, 12, 40):
        for i in np.nonzero(runs[A][0] == 0)[0]:
            batch.append(inst[i])
            regions.append(pm.words(runs[A][5][i]))
    plen = np.array([len(r) for r in regions], dtype=np.int64)
    stats = {}
    return batch, regions, plen, trim_all(batch, np.zeros(len(batch), dtype=np.int8), regions, plen, stats=stats), stats


MALFORMED = ('negative-length', 'long-length', 'variable', 'negative-literal')


def malform(inst, lemmas, kind, at):
    "the words of ``lemmas`` with lemma ``at`` malformed"
    import exact_proof_model as pm
    w = pm.words(lemmas)
    pos = sum(len(x) + 1 for x in lemmas[:at])
    if kind == 'negative-length':
        w[pos] = -1
    elif kind == 'long-length':
        w[pos] = len(w) - pos                                                       # one word more than is left
    elif kind == 'variable':
        w[pos + 1] = inst[0] << 1
    else:
        w[pos + 1] = -2
    return w


@functools.lru_cache(maxsize=None)
def mutation_batch():
    """One batch of every kind of input the entry point meets: (instances, status, regions, proof_len, trim_all of them, statistics, the
    forward verdicts where exact_proof_model recorded one, else None).  The mutated proofs of exact_proof_model.mutation_cases(); forged
    proofs of satisfiable instances; malformed lemmas; statuses that are not judged and proof_len outside the region; a tautological
    lemma in front of a genuine proof."""
    import exact_proof_model as pm
    inst, status, regions, plen, forward = [], [], [], [], []

    def add(ic, st, region, ln=None, fwd=None):
        inst.append(ic); status.append(st); regions.append(np.asarray(region, dtype=np.int32))
        plen.append(len(region) if ln is None else ln); forward.append(fwd)

    cases = pm.mutation_cases()
    for c in cases:
        add(c['inst'], 0, pm.words(c['mutated']), fwd=c['verdict'])
    genuine = [c for c in cases if c['kind'] == 'genuine' and len(c['lemmas']) >= 2]
    for k, c in enumerate(genuine[:16]):
        at = (0, len(c['lemmas']) - 1, len(c['lemmas']) // 2)[k % 3]
        add(c['inst'], 0, malform(c['inst'], c['lemmas'], MALFORMED[k % 4], at))
    for c in genuine[:6]:
        w = pm.words(c['lemmas'])
        add(c['inst'], 1, w)                                                         # a model needs no core
        add(c['inst'], -1, w)
        add(c['inst'], 0, w, -1)
        add(c['inst'], 0, w, len(w) + 1)
        add(c['inst'], 0, np.concatenate([w, [7, 7, 7]]), len(w))                   # the region is larger than the proof
        add(c['inst'], 0, pm.words([[0, 1]] + c['lemmas'] + [[2, 4, 3]]))           # tautologies: one nobody needs, one never reached
    # a lemma that does not follow but that nobody needs: the forward check refutes the proof, the backward check never looks at it
    for c in genuine[:8]:
        n, cl = c['inst']
        for L in range(2 * n):
            w = pm.words([[L, (L + 2) % (2 * n)]] + c['lemmas'])                    # in front: after a whole proof every clause follows
            if pm.check(n, cl, 0, None, w, len(w))[0] == 0 and trim(n, cl, w, len(w))[0] == 1:
                add(c['inst'], 0, w, fwd=0)
                break
    base, runs = pm.base_inputs()
    sat = [i for i in range(0, len(base), 6) if runs[0][0][i] == 1 and base[i][0] >= 2]
    for i in sat[:20]:
        for proof in ([], runs[0][5][i], [[0], [1]], [[0], [2], [1]]):               # forged: a satisfiable instance passed with status 0
            add(base[i], 0, pm.words(proof))
    add(cases[0]['inst'], 0, pm.words(cases[0]['lemmas']), fwd=1)                    # a mutated instance is never the last of the batch
    plen = np.array(plen, dtype=np.int64)
    stats = {}
    return inst, np.array(status, dtype=np.int8), regions, plen, trim_all(inst, status, regions, plen, stats=stats), stats, forward


# ---- past one wave's width: more than 64 units in one pass, literals in a reason, in a start clause and in a checked lemma, lemmas kept and
# lemmas skipped (the learning search's wide instances are satisfiable or undecided, so their proofs never reach a closure) -----------------
def wide_refutation(D, junk):
    """(instance, lemmas).  Variables a_0 .. a_{D-1}, y, z, u.  Clauses: the units a_i; W = (-a_0 .. -a_{D-1} y u); (-y z u); (-y -z u); (-u).
    The lemma X = (-a_0 .. -a_{D-1} u) follows through W as the reason of y (a reason of D + 2 literals met by one lane) and refutes the
    instance as the falsified clause of the empty clause's second pass (a start clause of D + 1 literals, after a pass of D + 1 units).
    ``junk`` satisfied lemmas (a_k y) stand before and after X: nobody needs them, the backward walk skips them."""
    a = list(range(1, D + 1))
    y, z, u = D + 1, D + 2, D + 3
    clauses = [[v] for v in a] + [[-v for v in a] + [y, u], [-y, z, u], [-y, -z, u], [-u]]
    code = lambda l: ((abs(l) - 1) << 1) | (1 if l < 0 else 0)
    filler = [[code(a[k % D]), code(y)] for k in range(junk)]
    return (D + 3, clauses), filler + [[code(-v) for v in a] + [code(u)]] + filler


def chain_refutation(K):
    """(instance, lemmas).  Clauses (b_0), (-b_k b_{k+1}) for k < K, (-b_K); lemmas (b_1) .. (b_K) in order.  Lemma k is refuted by lemma
    k - 1 and one clause (b_{k-1} is asked for in both polarities in a pass of k units), so all K lemmas are kept, each needed by the next."""
    clauses = [[1]] + [[-(k + 1), k + 2] for k in range(K)] + [[-(K + 1)]]
    return (K + 1, clauses), [[(k << 1)] for k in range(1, K + 1)]


@functools.lru_cache(maxsize=None)
def wide_cases():
    "(instances, regions, proof_len, the trim_all of them, statistics): wide_refutation at D = 70, 100 and 130, chain_refutation(150)"
    import exact_proof_model as pm
    made = [wide_refutation(70, 0), wide_refutation(100, 70), wide_refutation(130, 5), chain_refutation(150), wide_refutation(65, 200)]
    inst = [x[0] for x in made]
    regions = [pm.words(x[1]) for x in made]
    plen = np.array([len(r) for r in regions], dtype=np.int64)
    stats = {}
    return inst, regions, plen, trim_all(inst, np.zeros(len(inst), dtype=np.int8), regions, plen, stats=stats), stats
