"""Proofs of unsatisfiability from the learning complete search and their forward check (pdp_exact_solve_learn_proof and pdp_exact_check,
include/pdp_hip.h) stated in plain Python, in two independent parts.

(i)  ``search``: tests/exact_learn_model.py's search, pass for pass, with one addition: every learned clause that is stored in the arena is
     also appended to a lemma log, as literal codes (v << 1) | negative in the order the arena gets them (the negated UIP, then the other
     variables ascending).  ``proof_len`` is the number of words the log needs (len + 1 per lemma); ``region`` cuts the log to what a region
     of a given size receives.
(ii) ``check``: the checker.  It shares no code with (i): a model is checked clause by clause, a proof lemma by lemma for a refutation by
     unit propagation, with the words of the region treated as untrusted input.  It counts the same clause-literal reads as the GPU, so
     verdict, fail_at and work can be compared with array_equal."""
import functools

import numpy as np

from exact_model import NO_BUDGET, check_reads, hint_codes


# ---- (i) the learning search with its lemma log ---------------------------------------------------------------------------------------
def search(n, clauses, hints=None, budget=NO_BUDGET, arena=0):
    """(status, model, work, learned, reductions, lemmas, proof_len) of the instance: the first five are exact_learn_model.search's;
    lemmas = the stored learned clauses in order, each a list of literal codes; proof_len = sum(len + 1)."""
    if budget <= 0:
        budget = 1 << 32
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    cls = [[(abs(l) - 1, 2 if l < 0 else 1) for l in c] for c in clauses]        # (variable, the value that makes the literal true)
    m0 = len(cls)
    if arena <= 0:
        arena = 4 * sum(len(c) for c in cls)
    n = max([n] + [v + 1 for c in cls for v, _ in c])
    code = hint_codes(n, hints)
    zeros = np.zeros(n, dtype=np.float32)
    work = learned = reductions = used = 0
    lemmas = []

    def done(status, model):
        return status, model, work, learned, reductions, lemmas, sum(len(x) + 1 for x in lemmas)

    if all(code):                                                                 # the check pass: every variable has a hint
        bits = [1.0 if c == 1 else 0.0 for c in code]
        reads, ok = check_reads(clauses, bits)
        work += reads
        if ok:
            return done(1, np.asarray(bits, dtype=np.float32))
    val, lev, rsn = [0] * n, [0] * n, [None] * n
    trail, mark = [], {}
    level = 0
    while True:
        if work >= budget:
            return done(-1, zeros)
        # one unit-propagation pass: the lowest falsified clause, and per literal the lowest clause that asks for it
        confl, req, wmin = None, {}, None
        for ci, c in enumerate(cls):
            nfree, sat, first, distinct, k = 0, False, None, False, 0
            for L in c:
                k += 1
                x = val[L[0]]
                if x == 0:
                    if nfree == 0:
                        first = L
                    elif L != first:
                        distinct = True
                    nfree += 1
                elif x == L[1]:
                    sat = True
                    break
            work += k
            if sat:
                continue
            if nfree == 0:
                if confl is None:
                    confl = ci
            elif not distinct:
                req.setdefault(first, ci)
            else:
                wmin = nfree if wmin is None else min(wmin, nfree)
        if confl is None and req:
            asked = sorted({v for v, _ in req})
            both = [v for v in asked if (v, 1) in req and (v, 2) in req]
            for v in asked:
                if both and v == both[0]:
                    val[v], rsn[v], confl = 1, req[(v, 1)], req[(v, 2)]
                elif v in both:
                    continue
                else:
                    val[v] = 1 if (v, 1) in req else 2
                    rsn[v] = req[(v, val[v])]
                lev[v] = level
                trail.append(v)
            if confl is None:
                continue
        if confl is not None:
            if level == 0:
                return done(0, zeros)
            # first-UIP analysis: resolve backwards along the trail until one literal of the current level is left
            seen, out, open_, i, uip = set(), [], 0, len(trail) - 1, None
            c = cls[confl]
            while True:
                work += len(c)
                for v, p in c:
                    if v in seen:
                        continue
                    seen.add(v)
                    if lev[v] == level:
                        open_ += 1
                    elif lev[v] > 0:
                        out.append((v, p))
                while i >= 0 and trail[i] not in seen:
                    i -= 1
                assert i >= 0, "a conflict clause without a literal of the current level"
                uip = trail[i]
                i -= 1
                open_ -= 1
                if open_ == 0:
                    break
                c = cls[rsn[uip]]
            lc = [(uip, 3 - val[uip])] + sorted(out)
            bl = max([lev[v] for v, _ in out], default=0)
            for u in trail[mark[bl + 1]:]:
                val[u] = 0
            del trail[mark[bl + 1]:]
            level = bl
            if used + len(lc) + 1 > arena:
                # delete every learned clause that is not the reason of an assigned variable, keep the order, renumber; nothing is logged
                reasons = {rsn[v] for v in trail if rsn[v] is not None}
                remap, kept = {}, []
                for ci, c2 in enumerate(cls):
                    if ci < m0 or ci in reasons:
                        remap[ci] = len(kept)
                        kept.append(c2)
                cls = kept
                for v in trail:
                    if rsn[v] is not None:
                        rsn[v] = remap[rsn[v]]
                used = sum(len(c2) + 1 for c2 in cls[m0:])
                reductions += 1
                if used + len(lc) + 1 > arena:
                    return done(-1, zeros)                                        # the clause is not stored, so it is not logged either
            cls.append(lc)
            lemmas.append([(v << 1) | (1 if p == 2 else 0) for v, p in lc])
            used += len(lc) + 1
            learned += 1
            continue
        if wmin is None:
            return done(1, np.asarray([1.0 if x == 1 else 0.0 for x in val], dtype=np.float32))
        # branching: the unassigned variable with the most occurrences in the open clauses of minimum width, ties to the lower index
        cnt = {}
        for c in cls:
            nfree, sat, k = 0, False, 0
            for L in c:
                k += 1
                x = val[L[0]]
                if x == 0:
                    nfree += 1
                elif x == L[1]:
                    sat = True
                    break
            work += k
            if sat or nfree != wmin:
                continue
            for L in c:
                if val[L[0]] == 0:
                    cnt[L] = cnt.get(L, 0) + 1
            work += len(c)
        score = {}
        for (v, _), k in cnt.items():
            score[v] = score.get(v, 0) + k
        v = max(score, key=lambda u: (score[u], -u))
        positive = cnt.get((v, 1), 0) >= cnt.get((v, 2), 0)
        if code[v]:
            positive = code[v] == 1
        level += 1
        mark[level] = len(trail)
        val[v], lev[v], rsn[v] = (1 if positive else 2), level, None
        trail.append(v)


def words(lemmas):
    "the lemmas as the int32 words of a proof region: len, lit_0 .. lit_{len-1} per lemma"
    return np.asarray([w for x in lemmas for w in [len(x)] + list(x)], dtype=np.int32)


def region(lemmas, size):
    "the words a region of ``size`` words receives: whole lemmas in order up to the first one that does not fit, nothing after it"
    out = []
    for x in lemmas:
        if len(out) + len(x) + 1 > size:
            break
        out += [len(x)] + list(x)
    return np.asarray(out, dtype=np.int32)


def parse(region_words):
    "lemmas of well-formed region words (the inverse of ``words``)"
    w, out, pos = [int(x) for x in region_words], [], 0
    while pos < len(w):
        out.append(w[pos + 1:pos + 1 + w[pos]])
        pos += 1 + w[pos]
    assert pos == len(w)
    return out


def solve(instances, hints=None, budget=NO_BUDGET, arena=0):
    "search() over a list: (status, models, work, learned, reductions, lemma lists, proof_len int64 [N])"
    out = [search(n, c, None if hints is None else hints[i], budget, arena) for i, (n, c) in enumerate(instances)]
    return (np.array([o[0] for o in out], dtype=np.int8), [o[1] for o in out], np.array([o[2] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int32), np.array([o[4] for o in out], dtype=np.int32), [o[5] for o in out],
            np.array([o[6] for o in out], dtype=np.int64))


# ---- (ii) the checker -------------------------------------------------------------------------------------------------------------------
def _scan(lits, val):
    """one clause (literal codes) under val (0 unassigned, 1 true, 2 false): (reads, kind, literal) with kind 'sat', 'conflict',
    'unit' (literal = the one asked for) or 'open'; the clause is read up to and including its first true literal"""
    free = []
    for k, L in enumerate(lits):
        x = val[L >> 1]
        if x == 0:
            free.append(L)
        elif x == 1 + (L & 1):
            return k + 1, 'sat', None
    if not free:
        return len(lits), 'conflict', None
    if all(L == free[0] for L in free):
        return len(lits), 'unit', free[0]
    return len(lits), 'open', None


def check(n, clauses, status, model, region_words, proof_len, budget=0):
    """(verdict 1 / 0 / -1, fail_at, work) of one instance.  ``region_words``: the whole region of the instance (int32 words, any content);
    ``proof_len``: the words of it that are said to hold lemmas."""
    clauses = [[int(l) for l in c if int(l) != 0] for c in clauses]
    n = max([n] + [abs(l) for c in clauses for l in c])
    if budget <= 0:
        budget = 1 << 32
    if status not in (0, 1) or proof_len < 0 or proof_len > len(region_words):
        return -1, -1, 0
    if status == 1:
        work, fail = 0, -1                                                        # every clause is read, also after a failing one
        for ci, c in enumerate(clauses):
            k = next((j + 1 for j, l in enumerate(c) if (float(model[abs(l) - 1]) > 0.5) == (l > 0)), None)
            work += len(c) if k is None else k
            if k is None and fail < 0:
                fail = ci
        return (1 if fail < 0 else 0), fail, work
    orig = [[((abs(l) - 1) << 1) | (1 if l < 0 else 0) for l in c] for c in clauses]
    w = [int(x) for x in region_words[:proof_len]]
    lemmas, pos, work, i = [], 0, 0, 0
    while True:
        # lemma i, validated before it is used; i == L is the empty clause
        if pos < proof_len:
            ln = w[pos]
            if ln < 0 or pos + 1 + ln > proof_len:
                return 0, i, work
            lits = w[pos + 1:pos + 1 + ln]
            if any(L < 0 or (L >> 1) >= n for L in lits):
                return 0, i, work
            last = False
        else:
            lits, last = [], True
        val = [0] * n
        work += len(lits)
        taut = False
        for L in lits:
            f = 2 - (L & 1)                                                       # the value that makes L false
            if val[L >> 1] not in (0, f):
                taut = True
            val[L >> 1] = f
        accepted = taut
        while not accepted:
            if work >= budget:
                return -1, -1, work
            conflict, req = False, set()
            for c in orig + lemmas:
                reads, kind, L = _scan(c, val)
                work += reads
                if kind == 'conflict':
                    conflict = True
                elif kind == 'unit':
                    req.add(L)
            if conflict or any(L ^ 1 in req for L in req):
                accepted = True
            elif not req:
                return 0, i, work
            else:
                for L in req:
                    val[L >> 1] = 1 + (L & 1)
        if last:
            return 1, -1, work
        lemmas.append(lits)
        pos += 1 + len(lits)
        i += 1


def check_all(instances, status, models, regions, proof_len, budget=0):
    "check() over a list: (verdict int8 [N], fail_at int32 [N], work int64 [N])"
    out = [check(n, c, int(status[i]), models[i], regions[i], int(proof_len[i]), budget) for i, (n, c) in enumerate(instances)]
    return (np.array([o[0] for o in out], dtype=np.int8), np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.int64))


# ---- seeded mutations of a proof (lists of lemmas) -------------------------------------------------------------------------------------
MUTATIONS = ('flip', 'shrink', 'drop-first', 'drop-last', 'reverse', 'empty')


def mutate(lemmas, kind, rng):
    "a mutated copy; ``rng`` picks the lemma of 'flip' (sign of its first literal) and 'shrink' (cut to its first literal)"
    out = [list(x) for x in lemmas]
    if kind in ('flip', 'shrink') and out:
        j = int(rng.randint(len(out)))
        out[j] = [out[j][0] ^ 1] + out[j][1:] if kind == 'flip' else out[j][:1]
    elif kind == 'drop-first':
        out = out[1:]
    elif kind == 'drop-last':
        out = out[:-1]
    elif kind == 'reverse':
        out = out[::-1]
    elif kind == 'empty':
        out = []
    return out


# ---- the inputs shared by test_exact_proof_host.py and test_exact_proof_gpu.py: computed once per process, never modified by a test ----
def threshold(count, n, seed):
    "uniform 3-SAT at 4.26 clauses per variable"
    rng = np.random.RandomState(seed)
    inst = []
    for _ in range(count):
        clauses = []
        for _ in range(int(round(4.26 * n))):
            vs = rng.choice(n, size=3, replace=False) + 1
            clauses.append([int(v) * int(s) for v, s in zip(vs, rng.choice([-1, 1], size=3))])
        inst.append((n, clauses))
    return inst


@functools.lru_cache(maxsize=None)
def base_inputs():
    "(the small instances of the learning tests, families.exact_cases() and thrash 2 .. 12; arena -> solve() of them)"
    import exact_learn_model as lm
    import families
    from test_exact_learn_host import small_instances
    inst = small_instances() + [(n, c) for _, n, c in families.exact_cases()] + [lm.thrash(k) for k in range(2, 13)]
    return inst, {A: solve(inst, arena=A) for A in (0, 12, 40)}


MUTATION_SEED = 5


@functools.lru_cache(maxsize=None)
def mutation_cases():
    """The unsatisfiable runs of thrash 2 .. 12 and of threshold instances at n = 30 and n = 50, at arenas 0 and 40, each with every
    mutation of its proof: a list of dicts (inst, arena, lemmas, kind, mutated, verdict, fail_at, work), the last three from check()."""
    import exact_learn_model as lm
    inst = [lm.thrash(k) for k in range(2, 13)] + threshold(24, 30, 21) + threshold(12, 50, 12)
    rng = np.random.RandomState(MUTATION_SEED)
    out = []
    for arena in (0, 40):
        run = solve(inst, arena=arena)
        for i, (n, c) in enumerate(inst):
            if run[0][i] != 0:
                continue
            for kind in ('genuine',) + MUTATIONS:
                mut = run[5][i] if kind == 'genuine' else mutate(run[5][i], kind, rng)
                w = words(mut)
                v = check(n, c, 0, run[1][i], w, len(w))
                out.append(dict(inst=(n, c), arena=arena, lemmas=run[5][i], kind=kind, mutated=mut, verdict=v[0], fail_at=v[1], work=v[2]))
    return out
