"""SAT / UNSAT labels from the batched complete solver on the GPU (pdp_exact_solve and pdp_exact_solve_hinted, include/pdp_hip.h; DESIGN.md "Complete solver").

PDP is incomplete: it finds assignments but never proves an instance unsatisfiable, so the reference leaves labelling to "your SAT solver
of choice" (src/pdp/generator.py:15-17).  This module fills that hook: ``label_clause_lists`` labels many instances in a few launches,
``is_sat`` has the reference hook's signature, ``solve_items`` works on loader items.  A label is True (satisfiable), False
(unsatisfiable) or None (undecided within the budget of clause-literal reads per instance; 0 = the library default, 2^32).
With ``certify=True`` every answer is checked on the GPU before it becomes a label: a model against the clauses, an "unsatisfiable" by a
forward check of the learning search's learned clauses as a proof (pdp_exact_solve_learn_proof, pdp_exact_check);
``drat_lines`` writes such a proof for an external checker.  With ``cores=True`` the "unsatisfiable" answers are judged by the backward
check instead (pdp_exact_trim), which also says why: the core, the original clauses the refutation rests on, and the
lemmas it needs (``core_clauses``, ``trimmed``).  With ``assume=`` the question is "satisfiable with these literals held fixed, and if not,
which of them are to blame" (pdp_exact_solve_learn_assume); ``backbone`` asks it once per variable of every satisfiable
instance, in one batch: the literals that hold in every model.  ``min_unsat`` optimises instead of deciding: the fewest clauses any
assignment leaves unsatisfied, by branch and bound from a given assignment (pdp_exact_min_unsat) -- what an incomplete
solver's ``unsat_clauses`` on an unsatisfiable instance is to be compared with.  ``count_models`` counts instead of deciding: the exact
number of models of an instance and, per variable, the share of them in which it is true (pdp_exact_count) -- what PDP's
soft prediction is to be compared with.  With ``split=`` the deciding search of every instance is spread over 2^depth waves
(pdp_exact_solve_split): same labels and models, for the one hard instance that would otherwise occupy one wave of the GPU.
``count_models(split=)`` does the same for the count (pdp_exact_count_split): cube counts add, so the tail of a batch and a
single instance get the whole GPU, with the same counts and marginals.  ``min_unsat(split=)`` spreads the branch and bound
(pdp_exact_min_unsat_split): the cubes of an instance share the best cost found, so one cube's incumbent prunes all the
others; a proved cost is the same minimum, which minimiser comes back depends on the timing of the cubes.  ``models_at`` turns the
count into the models themselves: the counting search meets its satisfying cubes in a fixed order, so "count before the cube + offset inside it" numbers every model once, and
a rank becomes a model by walking that order with a cursor (pdp_exact_models_at) -- ``enumerate_models`` lists the first
models of an instance, ``sample_models`` draws uniformly from all of them (uniform ranks below the exact count): what PDP's own solution
is to be compared with, and a supervised target the marginals alone do not give.  ``solution_mass`` weighs instead of counting: the
probability that rounding every variable independently with a soft prediction gives a model, the posterior under that product prior,
and, where the budget ran out, the mass of the part of the tree not visited (pdp_exact_mass).
``solution_mass(split=)`` spreads that search over 2^depth waves as well (pdp_exact_mass_split): cube masses and open
masses add, the budget applies per cube, so a bracket is tightened by 2^depth times the reads.  ``mass_logit_gradient`` is the exact
gradient of -ln(mass) in the logits of the prediction, from the posterior.  ``nearest_model`` measures an assignment instead: the model
with the fewest variables (or the least sum of per-variable penalties) different from it, by branch and bound with every clause hard
(pdp_exact_nearest) -- how far PDP's assignment was from a solution, and which one; ``map_penalties`` turns a soft
prediction into the hint and penalties under which that model is the most probable one.  ``nearest_model(split=N)`` spreads that
search over 2^N waves per instance that share the best cost found, and ``start`` gives it models the caller already has to start below
(pdp_exact_nearest_split).
"""

import numpy as np
import torch

from pdp import native
from pdp.factorgraph import dataset

MAX_EDGES = 1 << 24          # edges per problem handed to the library
COUNT_MAX_N = 1023           # pdp_exact_count searches instances of up to this many variables (2^n is a finite double)
MAX_RANK = 1 << 53           # pdp_exact_models_at: ranks lie below (every rank and every count it is compared with is an exact double)
SPLIT_MAX_DEPTH = 16        # pdp_exact_solve_split: at most 2^16 cubes per instance
SPLIT_WAVES_PER_SIMD = 4     # k_exact_split's occupancy by registers (resources); four SIMDs per CU
# split='auto': the reads per instance of the plain first stage, and how many cubes the second stage makes per resident wave.  Chosen from
# the sweep in profiles/exact_time.txt ("split='auto' constants", tools/exact_time.py sweep)
AUTO_STAGE1_BUDGET = 1 << 18
AUTO_CUBES_PER_WAVE = 16
# count_models(split='auto'): the reads per instance of the plain first count.  Chosen from the sweep in profiles/exact_time.txt
# (tools/exact_time.py cssweep)
AUTO_COUNT_STAGE1_BUDGET = 1 << 26
# count_models(split='rounds'): the reads per cube and round (the library's default, PDP_EXACT_ROUND_BUDGET) and the most levels a stopped
# cube gives away in one expansion.  Chosen from the sweep in profiles/exact_time.txt (tools/exact_time.py crsweep): on
# row ca 2^18 is the fastest of 2^16 .. 2^24 at every cap of 4 and above, and the caps 4 / 8 / 16 differ by less than their spread.
# ROUNDS_WAVES_PER_SIMD is k_exact_count_round's occupancy by registers (resources)
ROUND_BUDGET = 1 << 18
ROUNDS_MAX_GIVE = 8
ROUNDS_WAVES_PER_SIMD = 3
DEFAULT_BUDGET = 1 << 32     # PDP_EXACT_DEFAULT_BUDGET
# solve_items(split='rounds'): the same three for the deciding search (the library's PDP_EXACT_SOLVE_ROUND_BUDGET).  Chosen from the sweep
# in profiles/exact_time.txt (tools/exact_time.py srsweep); SOLVE_ROUNDS_WAVES_PER_SIMD is k_exact_solve_round's
# occupancy by registers (resources)
SOLVE_ROUND_BUDGET = 1 << 18
SOLVE_ROUNDS_MAX_GIVE = 8
SOLVE_ROUNDS_WAVES_PER_SIMD = 4
# min_unsat(split='auto'): the reads per instance of the plain first branch and bound.  Chosen from the sweep in profiles/exact_time.txt
# (tools/exact_time.py xsweep)
AUTO_MIN_STAGE1_BUDGET = 1 << 26
# solution_mass(split='auto'): the reads per instance of the plain first mass.  The count's value: the tree at weights 0.5 is the count's
# (tools/exact_time.py zssweep sweeps it)
AUTO_MASS_STAGE1_BUDGET = 1 << 26
# nearest_model(split='auto'): the reads per instance of the plain first search.  Chosen from the sweep in profiles/exact_time.txt
# (tools/exact_time.py nssweep: the fastest of 2^18 / 2^22 / 2^26 on row nd; on row na, whose instances finish near 2^22 reads, it makes
# 'auto' 2.0 times the plain call where 2^26 is free: DESIGN.md §9.16 weighs the two)
AUTO_NEAREST_STAGE1_BUDGET = 1 << 22
# nearest_model_rounds: the reads per cube and round (the library's PDP_EXACT_NEAREST_ROUND_BUDGET), the most levels a stopped
# cube gives away in one expansion, and k_exact_nearest_round's occupancy by registers (resources and measured;
# tools/exact_time.py nrsweep sweeps the first two)
NEAREST_ROUND_BUDGET = 1 << 18
NEAREST_ROUNDS_MAX_GIVE = 8
NEAREST_ROUNDS_WAVES_PER_SIMD = 4


def raw_item(n, clauses, label=-1.0, name=""):
    """Loader item of an instance exactly as given: variables 1..n (also unused ones; more if a literal names a larger variable), every
    clause in order with its literals as written -- repeated literals, tautologies and empty clauses included.  (dataset.instance_from_clauses
    canonicalises like the reference's DIMACS converter: it drops empty clauses and keeps one literal per variable, which can change the
    answer.)  A DIMACS terminator 0 inside a clause is skipped."""
    rows = [[int(l) for l in c if int(l) != 0] for c in clauses]
    sv = np.asarray([l for r in rows for l in r], dtype=np.int64)
    ci = np.asarray([i for i, r in enumerate(rows) for _ in r], dtype=np.int64)
    n = max(int(n), int(np.abs(sv).max()) if sv.size else 0)
    graph_map = np.stack((np.abs(sv) - 1, ci)).astype(np.int32).reshape(2, -1)
    return n, len(rows), graph_map, np.sign(sv).astype(np.float32), float(label), [name] if name else []


def _segments(items, max_edges):
    "consecutive runs of items with at most max_edges edges each (a larger item gets a run of its own)"
    runs, cur, edges = [], [], 0
    for i, it in enumerate(items):
        e = int(it[2].shape[1])
        if cur and edges + e > max_edges:
            runs.append(cur)
            cur, edges = [], 0
        cur.append(i)
        edges += e
    if cur:
        runs.append(cur)
    return runs


def proof_lemmas(words):
    "the lemmas of a complete proof region (int32 words ``len, lit_0 .. lit_{len-1}`` per lemma) as lists of literal codes (v << 1) | negative"
    w, out, pos = [int(x) for x in words], [], 0
    while pos < len(w):
        if w[pos] < 0 or pos + 1 + w[pos] > len(w):
            raise ValueError("proof words: lemma %d does not fit the %d words given" % (len(out), len(w)))
        out.append(w[pos + 1:pos + 1 + w[pos]])
        pos += 1 + w[pos]
    return out


def drat_lines(lemmas):
    """A proof (lemmas as lists of literal codes, proof_lemmas) as DRAT text for an external checker: one line per lemma, signed 1-based
    literals terminated by 0, then the empty clause.  The searches never delete a clause from the proof, so there are no ``d`` lines."""
    lines = [' '.join([str(-((L >> 1) + 1) if L & 1 else (L >> 1) + 1) for L in lemma] + ['0']) for lemma in lemmas]
    return lines + ['0']


def trimmed(proof, proof_off, proof_len, keep):
    """The kept lemmas of Problem.exact_trim, compacted on the device: (words int32, offsets int64 [B+1]) -- instance b's kept lemmas, in
    order, are words[offsets[b] : offsets[b+1]], a complete proof in the format of ``proof``.  Only keep's bytes among the first
    proof_len[b] words of a region count, and a proof_len outside its region counts as none.  Nothing here knows a verdict: the kernel
    does not write the region of an instance it does not judge, so such an instance gets no words from the zeroed keep that exact_trim
    allocates, and whatever equals 1 there from a buffer the caller passed in -- mask by verdict then."""
    off = proof_off.reshape(-1).long()
    total = proof.numel()
    size = off[1:] - off[:-1]
    plen = torch.where((proof_len >= 0) & (proof_len <= size), proof_len, torch.zeros_like(proof_len))
    edge = torch.zeros(total + 1, dtype=torch.int64, device=proof.device)
    one = torch.ones_like(plen)
    edge.index_add_(0, off[:-1], one)
    edge.index_add_(0, off[:-1] + plen, -one)
    mask = (torch.cumsum(edge, 0)[:total] > 0) & (keep.reshape(-1) == 1)
    count = torch.cat([torch.zeros(1, dtype=torch.int64, device=proof.device), torch.cumsum(mask, 0)])
    return proof.reshape(-1)[mask], count[off]


def core_clauses(core, clauses_per_instance):
    "per instance the 0-based indices, in its own clause order, of its clauses with core = 1 (core: Problem.exact_trim's, one byte per clause)"
    core = core.cpu().numpy() if torch.is_tensor(core) else np.asarray(core)
    ends = np.cumsum(np.asarray(clauses_per_instance, dtype=np.int64))
    return [np.nonzero(part)[0] for part in np.split(core[:ends[-1]] if len(ends) else core[:0], ends[:-1])]


def _certified(prob, budget, hint, arena, names, proof_off=None, counts=None):
    """exact_solve_proof and exact_check of one problem: numpy (status, model, work, verdict, proof_len, region sizes, lemma lists of the
    unsatisfiable instances whose proof is complete, None elsewhere, core index arrays likewise).  A verdict 0 raises: the solver answered
    what its own evidence refutes.  ``counts`` (the clauses of every instance): the unsatisfiable instances are judged by exact_trim
    instead, the lemmas are the ones it keeps and the cores are filled in; None: no cores."""
    st, model, wk, _, proof, off, plen = prob.exact_solve_proof(budget, hints=hint, arena=arena, proof_off=proof_off)
    cores = [None] * prob.B
    if counts is None:
        verdict, fail_at, _ = prob.exact_check(st, model, proof, off, plen)
    else:
        # the models go through the forward check (it does not judge a status -1), the proofs through the backward one
        unsat = st == 0
        verdict, fail_at, _ = prob.exact_check(torch.where(unsat, torch.full_like(st, -1), st), model, proof, off, plen)
        tv, tf, _, core, keep, _, _ = prob.exact_trim(st, proof, off, plen)
        verdict, fail_at = torch.where(unsat, tv, verdict), torch.where(unsat, tf, fail_at)
        if proof is not None:
            proof, toff = trimmed(proof, off, plen, keep)
            toff = toff.cpu().numpy()
    st, model, wk, verdict, fail_at = st.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy(), verdict.cpu().numpy(), fail_at.cpu().numpy()
    off, plen = off.cpu().numpy(), plen.cpu().numpy()
    if counts is not None:
        cores = [c if st[j] == 0 and verdict[j] == 1 else None for j, c in enumerate(core_clauses(core, counts))]
    for j in np.nonzero(verdict == 0)[0]:
        raise RuntimeError("the complete solver's answer for instance %s (status %d) fails its own check at %s %d: a solver bug, no label is "
                           "written from it" % (names[j], st[j], 'clause' if st[j] == 1 else 'lemma', fail_at[j]))
    words = None if proof is None else proof.cpu().numpy()
    # where the lemmas of instance j lie: its region's first proof_len words, or, trimmed, its own run of the compacted words
    a, z = (off[:-1], off[:-1] + plen) if counts is None or proof is None else (toff[:-1], toff[1:])
    lemmas = [proof_lemmas(words[a[j]:z[j]]) if st[j] == 0 and verdict[j] == 1 and z[j] > a[j] else ([] if st[j] == 0 and verdict[j] == 1 else None)
              for j in range(len(st))]
    return st, model, wk, verdict, plen, off[1:] - off[:-1], lemmas, cores


def _problem(part, device):
    b = dataset.to_torch(dataset.collate_segment(part), device)
    return native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(part))


def _certified_part(prob, part, names, budget, hint, arena, device, cores):
    """_certified on the problem of ``part``; an instance whose proof did not fit its region is solved once more, in a batch of its own,
    with a region of exactly the size it reported.  (status, model, work, verdict, lemmas, cores) in numpy / lists."""
    counts = [int(it[1]) for it in part] if cores else None
    st, model, wk, vd, plen, size, lem, cor = _certified(prob, budget, hint, arena, names, counts=counts)
    again = [j for j in range(len(part)) if st[j] != -1 and plen[j] > size[j]]
    if again:
        prob = _problem([part[j] for j in again], device)
        voff = np.concatenate([[0], np.cumsum([int(it[0]) for it in part])])
        hint2 = None if hint is None else torch.cat([hint[voff[j]:voff[j + 1]] for j in again])
        off2 = torch.from_numpy(np.concatenate([[0], np.cumsum(plen[again])]).astype(np.int64)).to(device)
        r = _certified(prob, budget, hint2, arena, [names[j] for j in again], proof_off=off2,
                       counts=[counts[j] for j in again] if cores else None)
        for k, j in enumerate(again):
            vd[j], lem[j], cor[j] = r[3][k], r[6][k], r[7][k]
    return st, model, wk, vd, lem, cor


def with_units(item, literals):
    "the loader item with one unit clause more per signed 1-based literal (after its own clauses; nothing else changes)"
    n, m, gm, ef = int(item[0]), int(item[1]), np.asarray(item[2]), np.asarray(item[3])
    lits = np.asarray(literals, dtype=np.int64).reshape(-1)
    more = np.stack((np.abs(lits) - 1, m + np.arange(lits.size))).astype(gm.dtype).reshape(2, -1)
    return (n, m + int(lits.size), np.concatenate([gm.reshape(2, -1), more], axis=1), np.concatenate([ef.reshape(-1), np.sign(lits).astype(ef.dtype)]),
            item[4], item[5])


def _assumed(prob, part, names, assume, budget, hint, arena, device, certify):
    """exact_solve_assume of one problem: numpy (status, model, work, verdict, lemmas, failed index arrays).  ``certify``: a model is
    checked by pdp_exact_check and against the assumptions; a status 0 by the refutation of the instance plus its failed assumptions as
    unit clauses, found and checked by the certified learning search in a batch of its own -- the learned clauses of a search under
    assumptions follow from the formula alone, so no new checker is needed.  A refuted answer raises RuntimeError."""
    st_t, model_t, wk_t, failed_t = prob.exact_solve_assume(budget, hints=hint, assume=assume, arena=arena)
    st, model, wk, fl = st_t.cpu().numpy(), model_t.cpu().numpy(), wk_t.cpu().numpy(), failed_t.cpu().numpy()
    voff = np.concatenate([[0], np.cumsum([int(it[0]) for it in part])])
    failed = [np.nonzero(fl[voff[j]:voff[j + 1]])[0].astype(np.int64) if st[j] == 0 else None for j in range(len(part))]
    verdict = np.full(len(part), -1, dtype=np.int8)
    lemmas = [None] * len(part)
    if not certify:
        return st, model, wk, verdict, lemmas, failed
    a = assume.cpu().numpy()
    none = torch.zeros(len(part), dtype=torch.int64, device=device)
    vd, fail_at, _ = prob.exact_check(torch.where(st_t == 1, st_t, torch.full_like(st_t, -1)), model_t, None,
                                      torch.zeros(len(part) + 1, dtype=torch.int64, device=device), none)
    vd, fail_at = vd.cpu().numpy(), fail_at.cpu().numpy()
    for j in np.nonzero(st == 1)[0]:
        if vd[j] != 1:
            raise RuntimeError("the complete solver's answer for instance %s (status 1) fails its own check at clause %d: a solver bug, no label "
                               "is written from it" % (names[j], fail_at[j]))
        aj, mj = a[voff[j]:voff[j + 1]], model[voff[j]:voff[j + 1]]
        bad = np.nonzero((aj != 0) & ((mj > 0.5) != (aj > 0)))[0]
        if bad.size:
            raise RuntimeError("the complete solver's model for instance %s disagrees with the assumption on variable %d: a solver bug, no "
                               "label is written from it" % (names[j], bad[0] + 1))
        verdict[j] = 1
    unsat = [int(j) for j in np.nonzero(st == 0)[0]]
    if unsat:
        reduced = []
        for j in unsat:
            aj = a[voff[j]:voff[j + 1]]
            if (aj[failed[j]] == 0).any():
                raise RuntimeError("the failed set of instance %s names a variable that is not assumed: a solver bug" % names[j])
            reduced.append(with_units(part[j], [(v + 1) if aj[v] > 0 else -(v + 1) for v in failed[j]]))
        rnames = ['%s with its failed assumptions' % names[j] for j in unsat]
        keep = [k for k, it in enumerate(reduced) if int(it[2].shape[1]) > 0]
        for k in set(range(len(unsat))) - set(keep):
            verdict[unsat[k]], lemmas[unsat[k]] = 1, []                # only empty clauses: an empty clause is its own refutation
        if keep:
            sub = [reduced[k] for k in keep]
            r = _certified_part(_problem(sub, device), sub, [rnames[k] for k in keep], budget, None, arena, device, False)
            for i, k in enumerate(keep):
                j = unsat[k]
                if r[0][i] == 1:
                    raise RuntimeError("the complete solver's answer for instance %s (status 0 under assumptions) is refuted: the instance "
                                       "with its failed assumptions as unit clauses is satisfiable; a solver bug, no label is written from it"
                                       % names[j])
                if r[0][i] == 0:
                    verdict[j], lemmas[j] = r[3][i], r[4][i]
    return st, model, wk, verdict, lemmas, failed


def auto_depth(undecided, device):
    """split='auto': the depth that gives ``undecided`` instances AUTO_CUBES_PER_WAVE cubes per resident wave of k_exact_split between them,
    clamp(floor(log2(target / undecided)), 0, SPLIT_MAX_DEPTH)"""
    waves = torch.cuda.get_device_properties(device).multi_processor_count * 4 * SPLIT_WAVES_PER_SIMD
    target = AUTO_CUBES_PER_WAVE * waves
    return max(0, min(SPLIT_MAX_DEPTH, (target // max(1, int(undecided))).bit_length() - 1))


def _check_split(split):
    if split is None or split == 'auto':
        return split
    if isinstance(split, bool) or not isinstance(split, (int, np.integer)) or not 0 <= split <= SPLIT_MAX_DEPTH:
        raise ValueError("split must be None, 'auto' or a depth from 0 to %d, got %r" % (SPLIT_MAX_DEPTH, split))
    return int(split)


def split_solve(prob, part, budget, hint, split, device):
    """The split search of one problem (``part``: its loader items, or a callable that returns them): numpy (status, model, work,
    depth_used).  ``split`` an int: one pdp_exact_solve_split call at that depth.  'auto': a plain exact_solve with AUTO_STAGE1_BUDGET reads
    per instance (``budget`` if that is smaller), then the undecided instances as one split call on a problem of their own at auto_depth;
    work is the sum of the two stages."""
    if split != 'auto':
        st, model, wk, _, du = prob.exact_solve_split(budget, hints=hint, depth=split, stats=True)[:5]
        return st.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy(), du.cpu().numpy()
    st, model, wk = prob.exact_solve(min(budget, AUTO_STAGE1_BUDGET) if budget > 0 else AUTO_STAGE1_BUDGET, hints=hint)
    st, model, wk = st.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy()
    du = np.zeros(len(st), dtype=np.int8)
    again = [int(j) for j in np.nonzero(st == -1)[0]]
    if again:
        depth = auto_depth(len(again), device)
        r = _on_their_own(part, again, device, lambda sub, cut: sub.exact_solve_split(budget, hints=cut(hint), depth=depth, stats=True)[:5],
                          {1: model})
        st[again], du[again] = r[0], r[4]
        wk[again] += r[2]
    return st, model, wk, du


def _on_their_own(part, which, device, call, per_variable):
    """Instances ``which`` (ascending indices) of a problem as a problem of their own.  ``part``: the loader items, or a callable that
    returns them.  call(sub, cut) runs on the new problem, cut(t) being the values of a per-variable tensor (or None) that belong to
    it; its tensors come back as numpy arrays.  ``per_variable`` {index of a result: array of the whole problem}: those results are
    written back into the instances' slices."""
    part = part() if callable(part) else part
    voff = np.concatenate([[0], np.cumsum([int(it[0]) for it in part])])
    sub = _problem([part[j] for j in which], device)
    r = [t.cpu().numpy() for t in call(sub, lambda t: None if t is None else torch.cat([t[int(voff[j]):int(voff[j + 1])] for j in which]))]
    del sub
    off = 0
    for j in which:
        n = int(voff[j + 1] - voff[j])
        for k, whole in per_variable.items():
            whole[voff[j]:voff[j + 1]] = r[k][off:off + n]
        off += n
    return r


def _rounds_give(open_cubes, device, waves_per_simd, max_give):
    """The levels every stopped cube gives away so that ``open_cubes`` of them become AUTO_CUBES_PER_WAVE cubes per resident wave of a
    round kernel that holds ``waves_per_simd``: the smallest g with open_cubes * (1 + g) >= that target, 0 once the frontier fills the
    GPU, capped by ``max_give`` and by the 2^22 cubes of a frontier"""
    waves = torch.cuda.get_device_properties(device).multi_processor_count * 4 * waves_per_simd
    target = AUTO_CUBES_PER_WAVE * waves
    open_cubes = max(1, int(open_cubes))
    give = -(-target // open_cubes) - 1
    return max(0, min(give, max_give, native.COUNT_ROUNDS_MAX_CUBES // open_cubes - 1))


def _drop_spent(state, total):
    """The total budget of a search in rounds, between two rounds: the cubes of every instance whose work has reached ``total`` (an int,
    or an int64 tensor of one value per instance on the state's device) leave the frontier; what the state holds of the instance
    stays.  Returns (the mask of the instances that left, their number); the number is the one host synchronisation."""
    per = state.cube_off[1:] - state.cube_off[:-1]
    spent = (state.work >= total) & (per > 0)
    left = int(spent.sum().item())
    if left:
        keep = ~torch.repeat_interleave(spent, per)
        state.len, state.bits, state.closed = state.len[keep].contiguous(), state.bits[keep].contiguous(), state.closed[keep].contiguous()
        state.cube_off = torch.cat([state.cube_off[:1], torch.cumsum(torch.where(spent, torch.zeros_like(per), per), 0)])
    return spent, left


def solve_rounds_give(open_cubes, device):
    """split='rounds' of the deciding search: rounds_give's rule with k_exact_solve_round's occupancy -- the smallest g with open_cubes *
    (1 + g) >= AUTO_CUBES_PER_WAVE cubes per resident wave, 0 once the frontier fills the GPU -- capped by SOLVE_ROUNDS_MAX_GIVE and by the
    2^22 cubes of a frontier"""
    return _rounds_give(open_cubes, device, SOLVE_ROUNDS_WAVES_PER_SIMD, SOLVE_ROUNDS_MAX_GIVE)


def solve_rounds(prob, part, budget, hint, round_budget, give, rounds, device):
    """The deciding search of one problem in rounds (Problem.exact_solve_round; ``part``: its loader items, or a callable that returns
    them, read only where an instance has more than 1023 variables): numpy (status, model, work, rounds_used int32).  Every round runs
    every open cube for ``round_budget`` reads past its replay (None or 0: SOLVE_ROUND_BUDGET) and cuts the frontier it leaves again,
    ``give`` levels per stopped cube (None: solve_rounds_give of the open cubes, every round).  ``budget`` is the total of reads per
    instance over all rounds and cubes (0: the library's default budget): an instance whose work has reached it leaves the frontier with
    status -1.  ``rounds``: at most so many rounds (None: until no cube is open); instances that are still open then end with status -1
    as well.  An instance of more than 1023 variables has no cube: it goes to the plain call, with ``budget``, and uses 0 rounds."""
    total = budget if budget > 0 else DEFAULT_BUDGET
    state = prob.exact_solve_begin(hint)
    done = 0
    while state.cubes and (rounds is None or done < rounds):
        prob.exact_solve_round(state, round_budget or SOLVE_ROUND_BUDGET, solve_rounds_give(state.cubes, device) if give is None else give)
        done += 1
        _drop_spent(state, total)                                                 # out of reads: the status stays -1
    st, model, wk, used = state.status.cpu().numpy(), state.model.cpu().numpy(), state.work.cpu().numpy(), state.rounds.cpu().numpy()
    wide = [int(j) for j in np.nonzero(st == -2)[0]]
    if wide:
        r = _on_their_own(part, wide, device, lambda sub, cut: sub.exact_solve(budget, hints=cut(hint)), {1: model})
        st[wide], wk[wide] = r[0], r[2]
    return st, model, wk, used


def solve_items(items, budget=0, device=None, max_edges=MAX_EDGES, hints=None, learn=False, arena=0, certify=False, proofs=False, cores=False,
                assume=None, split=None, round_budget=None, rounds=None):
    """Solve loader items ((n, m, graph_map, edge_feature, label, misc) tuples: dataset.instance_from_clauses, dataset.random_ksat_items,
    dataset.parse_line, raw_item).  Returns numpy (status int8 [N] in {1, 0, -1}, models: a float32 0/1 array of n_i values per instance,
    work int64 [N]).  Instances are packed into problems of at most ``max_edges`` edges; nothing couples two instances.
    ``hints``: per instance an array of n_i phase hints (> 0.5 true first, other finite values false first, NaN none) or None (no hints for
    that instance); the search is then pdp_exact_solve_hinted's (include/pdp_hip.h).
    ``learn``: the search with conflict clause learning (pdp_exact_solve_learn) and ``arena`` words per instance for its learned clauses
    (0: four per literal); same answers, far fewer reads on structured instances.
    ``certify``: the learning search with its lemma log (pdp_exact_solve_learn_proof), and every answer checked on the GPU (pdp_exact_check):
    a model against the clauses, an "unsatisfiable" by a forward check of the learned clauses as a proof.  Also returns verdict int8 [N]:
    1 checked, -1 not (undecided).  An instance whose proof did not fit its region is solved once more with a region of the size it
    reported.  A refuted answer raises RuntimeError naming the instance.  ``proofs`` (with certify): also return, per instance, the lemmas
    (lists of literal codes, see drat_lines) of a certified unsatisfiable instance and None for the others.
    ``cores`` (with certify): an "unsatisfiable" is judged by the backward check (pdp_exact_trim) in place of the forward one -- models
    still go through pdp_exact_check.  Returns (status, models, work, verdict, lemmas, cores): per certified unsatisfiable instance the
    lemmas the refutation needs (a proof against the core alone) and the 0-based indices of its core clauses, an unsatisfiable subset of
    the instance; None for the others.
    ``assume``: per instance an integer array of n_i values (> 0 the variable is held true, < 0 held false, 0 free) or None; the search is
    then the learning one under assumptions (pdp_exact_solve_learn_assume), which ``assume`` implies.  A status 1 means "satisfiable with
    these literals fixed" and its model agrees with them; the return value gains, as its last element, ``failed``: per status-0 instance
    the int64 array of the 0-based assumed variables that are to blame (the instance plus those assumptions as unit clauses is
    unsatisfiable; empty: it is unsatisfiable on its own), None for the others.  With ``certify`` a model is also checked against the
    assumptions, and an "unsatisfiable" by the certified refutation of the instance plus its failed assumptions as unit clauses
    (``proofs``: that refutation's lemmas).  ``cores`` under assumptions is not available.
    ``split``: the plain search (with ``hints`` if given) of every instance spread over 2^split waves (pdp_exact_solve_split; an int from 0
    to 16), or 'auto': see split_solve.  Status and models are those of the call without ``split`` while no cube runs out of ``budget``,
    which then applies to every cube; work is the sum over the cubes that count.  Not with ``learn``, ``certify`` or ``assume``.
    ``split='rounds'``: see solve_rounds -- the search in rounds of ``round_budget`` reads per cube, at most ``rounds`` of them, the open
    part of every tree cut again between two rounds to fill the GPU.  ``budget`` is then the total of reads per instance over all rounds
    and cubes; status is that of the call without ``split`` while the total is not reached, every model satisfies its instance, and which
    model comes back is not promised.  There is no check pass: a complete hint is followed, not tested first."""
    by_rounds = isinstance(split, str) and split == 'rounds'
    if not by_rounds:
        split = _check_split(split)
        if round_budget is not None or rounds is not None:
            raise ValueError("round_budget and rounds belong to split='rounds'")
    else:
        for name, x in (('round_budget', round_budget), ('rounds', rounds)):
            if x is not None and (isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1):
                raise ValueError("%s must be None or a positive integer, got %r" % (name, x))
    if split is not None and (learn or certify or assume is not None):
        raise ValueError("split spreads the plain search: pass it without learn, certify and assume")
    learn = learn or certify or assume is not None
    if cores and assume is not None:
        raise ValueError("cores under assumptions are not available: pass assume without cores")
    if proofs and not certify:
        raise ValueError("proofs belong to the certified search: pass certify=True")
    if cores and not certify:
        raise ValueError("cores belong to the certified search: pass certify=True")
    if arena and not learn:
        raise ValueError("arena belongs to the learning search: pass learn=True")
    native.require_gpu()
    if hints is not None:
        if len(hints) != len(items):
            raise ValueError("hints: one entry per instance (%d), got %d" % (len(items), len(hints)))
        for it, h in zip(items, hints):
            if h is not None and np.asarray(h).size != int(it[0]):
                raise ValueError("hints: instance %r has %d variables, its hints %d values" % (it[5], int(it[0]), np.asarray(h).size))
    if assume is not None:
        if len(assume) != len(items):
            raise ValueError("assume: one entry per instance (%d), got %d" % (len(items), len(assume)))
        for it, a in zip(items, assume):
            if a is not None and (np.asarray(a).size != int(it[0]) or np.asarray(a).dtype.kind not in 'iu'):
                raise ValueError("assume: instance %r has %d variables, its assumptions are %d values of type %s"
                                 % (it[5], int(it[0]), np.asarray(a).size, np.asarray(a).dtype))
        if isinstance(arena, bool) or not isinstance(arena, (int, np.integer)) or not 0 <= arena <= 1 << 30:
            raise ValueError("arena must be an integer from 0 to 2^30 words, got %r" % (arena,))
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    failed = [None] * N
    status = np.zeros(N, dtype=np.int8)
    work = np.zeros(N, dtype=np.int64)
    models = [None] * N
    verdict = np.full(N, -1, dtype=np.int8)
    lemmas = [None] * N
    core = [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere, so there is nothing to search (and no problem to build: the layout needs an edge): an instance without
            # clauses is satisfiable, one whose clauses are all empty is not
            for i, it in zip(seg, part):
                status[i] = 1 if int(it[1]) == 0 else 0
                verdict[i], lemmas[i] = 1, (None if status[i] else [])         # an empty clause is its own refutation
                core[i] = np.zeros(1, dtype=np.int64) if cores and not status[i] else None
                models[i] = np.zeros(int(it[0]), dtype=np.float32)
                h = None if hints is None or hints[i] is None else np.asarray(hints[i], dtype=np.float32).reshape(-1)
                if status[i] == 1 and h is not None and not np.isnan(h).any():
                    models[i] = (h > 0.5).astype(np.float32)           # the check pass accepts a complete hint: no clause objects
                if assume is not None:
                    a = np.zeros(int(it[0]), dtype=np.int8) if assume[i] is None else np.sign(np.asarray(assume[i]).reshape(-1)).astype(np.int8)
                    if status[i] == 1 and a.any():
                        # the assumptions are the codes of their variables: the check pass if every variable has one, else level 1
                        coded = h is not None and not (np.isnan(h) & (a == 0)).any()
                        models[i] = np.where(a != 0, a > 0, (h > 0.5) if coded else False).astype(np.float32)
                    failed[i] = None if status[i] else np.zeros(0, dtype=np.int64)
            continue
        with torch.cuda.device(device):
            prob = _problem(part, device)
            hint = None
            if hints is not None:
                flat = [np.full(int(it[0]), np.nan, dtype=np.float32) if hints[i] is None else np.asarray(hints[i], dtype=np.float32).reshape(-1)
                        for i, it in zip(seg, part)]
                hint = torch.from_numpy(np.concatenate(flat)).to(device)
            names = ['%d (%s)' % (i, ' '.join(str(x) for x in it[5])) if it[5] else str(i) for i, it in zip(seg, part)]
            if assume is not None:
                flat = [np.zeros(int(it[0]), dtype=np.int8) if assume[i] is None else np.sign(np.asarray(assume[i]).reshape(-1)).astype(np.int8)
                        for i, it in zip(seg, part)]
                st, model, wk, vd, lem, fl = _assumed(prob, part, names, torch.from_numpy(np.concatenate(flat)).to(device), budget, hint, arena,
                                                      device, certify)
                for j, i in enumerate(seg):
                    verdict[i], lemmas[i], failed[i] = vd[j], lem[j], fl[j]
            elif certify:
                st, model, wk, vd, lem, cor = _certified_part(prob, part, names, budget, hint, arena, device, cores)
                for j, i in enumerate(seg):
                    verdict[i], lemmas[i], core[i] = vd[j], lem[j], cor[j]
            elif by_rounds:
                st, model, wk, _ = solve_rounds(prob, part, budget, hint, round_budget, None, rounds, device)
            elif split is not None:
                st, model, wk, _ = split_solve(prob, part, budget, hint, split, device)
            else:
                st, model, wk = prob.exact_solve(budget, hints=hint, learn=learn, arena=arena)
                st, model, wk = st.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy()
        del prob
        off = 0
        for j, (i, it) in enumerate(zip(seg, part)):
            n = int(it[0])
            status[i], work[i] = st[j], wk[j]
            models[i] = model[off:off + n].copy()
            off += n
    if cores:
        return status, models, work, verdict, lemmas, core
    tail = () if assume is None else (failed,)
    if certify:
        return ((status, models, work, verdict, lemmas) if proofs else (status, models, work, verdict)) + tail
    return (status, models, work) + tail


def min_unsat_split(prob, part, budget, hint, split, device):
    """The split branch and bound of one problem (``part``: its loader items, or a callable that returns them; ``hint``: a float32 tensor
    of V values): numpy (status, cost, model, work, depth_used).  ``split`` an int: one pdp_exact_min_unsat_split call at that depth.
    'auto': a plain exact_min_unsat with AUTO_MIN_STAGE1_BUDGET reads per instance (``budget`` if that is smaller), then the instances
    whose optimum is not proved go through one split call on a problem of their own at auto_depth, with ``budget`` per cube.  The models
    of the first stage are the hints of that call -- an incumbent carries over, so the second stage starts from the first stage's cost;
    work is the sum of the two stages."""
    if split != 'auto':
        st, co, model, wk, _, _, du = prob.exact_min_unsat_split(budget, hints=hint, depth=split, stats=True)[:7]
        return st.cpu().numpy(), co.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy(), du.cpu().numpy()
    st, co, model, wk = prob.exact_min_unsat(min(budget, AUTO_MIN_STAGE1_BUDGET) if budget > 0 else AUTO_MIN_STAGE1_BUDGET, hints=hint)
    st, co, model, wk = st.cpu().numpy(), co.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy()
    du = np.zeros(len(st), dtype=np.int8)
    again = [int(j) for j in np.nonzero(st == -1)[0]]
    if again:
        part = part() if callable(part) else part
        voff = np.concatenate([[0], np.cumsum([int(it[0]) for it in part])])
        sub = _problem([part[j] for j in again], device)
        hint2 = torch.from_numpy(np.concatenate([model[voff[j]:voff[j + 1]] for j in again])).to(device)
        r = [t.cpu().numpy() for t in sub.exact_min_unsat_split(budget, hints=hint2, depth=auto_depth(len(again), device), stats=True)[:7]]
        del sub
        off = 0
        for k, j in enumerate(again):
            n = int(voff[j + 1] - voff[j])
            st[j], co[j], du[j] = r[0][k], r[1][k], r[6][k]
            wk[j] += r[3][k]
            model[voff[j]:voff[j + 1]] = r[2][off:off + n]
            off += n
    return st, co, model, wk, du


def min_unsat(items, budget=0, device=None, max_edges=MAX_EDGES, hints=None, split=None, depths=False):
    """The fewest unsatisfied clauses of loader items (as solve_items takes them) by branch and bound (pdp_exact_min_unsat).  Returns numpy
    (status int8 [N]: 1 the cost is the minimum over all assignments, -1 the budget ran out and it is an upper bound; cost int32 [N];
    models: per instance a float32 0/1 array of n_i values that leaves exactly cost clauses unsatisfied; work int64 [N]).
    ``hints``: per instance an array of n_i values or None -- the assignment the search starts from as its incumbent (> 0.5 true, every
    other value false, NaN included; None: all false), so cost never exceeds what that assignment leaves unsatisfied.
    ``split``: the search of every instance spread over 2^split waves that share the best cost found (pdp_exact_min_unsat_split; an int
    from 0 to 16), or 'auto': see min_unsat_split.  ``budget`` then applies to every cube.  A proved cost is the same minimum; which
    minimiser the model is and work depend on the timing of the cubes.  ``depths``: also return depth_used int8 [N]."""
    split = _check_split(split)
    native.require_gpu()
    if hints is not None:
        if len(hints) != len(items):
            raise ValueError("hints: one entry per instance (%d), got %d" % (len(items), len(hints)))
        for it, h in zip(items, hints):
            if h is not None and np.asarray(h).size != int(it[0]):
                raise ValueError("hints: instance %r has %d variables, its hints %d values" % (it[5], int(it[0]), np.asarray(h).size))
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    status = np.ones(N, dtype=np.int8)
    cost = np.zeros(N, dtype=np.int32)
    work = np.zeros(N, dtype=np.int64)
    used = np.zeros(N, dtype=np.int8)
    models = [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        flat = [np.zeros(int(it[0]), dtype=np.float32) if hints is None or hints[i] is None else np.asarray(hints[i], dtype=np.float32).reshape(-1)
                for i, it in zip(seg, part)]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere (and no problem to build: the layout needs an edge): every assignment leaves exactly the empty clauses
            # unsatisfied, the incumbent among them
            for i, it, h in zip(seg, part, flat):
                cost[i] = int(it[1])
                models[i] = (h > 0.5).astype(np.float32)
            continue
        with torch.cuda.device(device):
            prob = _problem(part, device)
            hint = torch.from_numpy(np.concatenate(flat)).to(device)
            if split is None:
                st, co, model, wk = prob.exact_min_unsat(budget, hints=hint)
                st, co, model, wk = st.cpu().numpy(), co.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy()
                du = np.zeros(len(part), dtype=np.int8)
            else:
                st, co, model, wk, du = min_unsat_split(prob, part, budget, hint, split, device)
        del prob
        off = 0
        for j, (i, it) in enumerate(zip(seg, part)):
            n = int(it[0])
            status[i], cost[i], work[i], used[i] = st[j], co[j], wk[j], du[j]
            models[i] = model[off:off + n].copy()
            off += n
    return (status, cost, models, work, used) if depths else (status, cost, models, work)


MAX_PENALTY = 1 << 20        # pdp_exact_nearest: a penalty is an integer in [0, MAX_PENALTY]


def map_penalties(weights, scale=1024):
    """(hints float32, penalties int32) of a soft prediction ``weights`` (probabilities of the variables being true, any shape) for
    nearest_model: hint = p > 0.5 and penalty = min(2^20, round(scale * |log p - log(1 - p)|)), computed in float64, with p = 0 or 1
    giving 2^20.  With these the nearest model is the model of highest probability under the product prior, up to the quantisation.
    NaN or a value outside [0, 1] raises."""
    p = np.asarray(weights, dtype=np.float64)
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("weights must be probabilities in [0, 1] without NaN")
    if not scale > 0:
        raise ValueError("scale must be positive, got %r" % (scale,))
    with np.errstate(divide='ignore'):
        gap = np.abs(np.log(p) - np.log1p(-p))
    pen = np.where(np.isfinite(gap), np.minimum(np.rint(scale * np.where(np.isfinite(gap), gap, 0.0)), MAX_PENALTY), MAX_PENALTY)
    return (p > 0.5).astype(np.float32), pen.astype(np.int32)


def nearest_split(prob, part, budget, hint, pen, start, split, device):
    """The split nearest-model search of one problem (``part``: its loader items, or a callable that returns them; ``hint``, ``pen``,
    ``start``: tensors of V values, the last two or None): numpy (status, cost, model, work, depth_used, start_cost).  ``split`` an int: one
    pdp_exact_nearest_split call at that depth.  'auto': a plain exact_nearest with AUTO_NEAREST_STAGE1_BUDGET reads per instance
    (``budget`` if that is smaller), then the instances whose optimum is not proved go through one split call on a problem of their own at
    auto_depth, with ``budget`` per cube.  The hint is the point the distance is measured from and stays; the models of the first stage are
    the start models of that call -- an incumbent carries over, so the second stage starts below the first stage's cost (where the first
    stage met no model, the caller's start model is passed on instead); work is the sum of the two stages."""
    if split != 'auto':
        r = prob.exact_nearest_split(hint, pen, start, depth=split, budget=budget, stats=True)
        st, co, model, wk, du, sc = r[0], r[1], r[2], r[3], r[6], r[7]
        return st.cpu().numpy(), co.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy(), du.cpu().numpy(), sc.cpu().numpy()
    stage1 = min(budget, AUTO_NEAREST_STAGE1_BUDGET) if budget > 0 else AUTO_NEAREST_STAGE1_BUDGET
    st, co, model, wk = [t.cpu().numpy() for t in prob.exact_nearest(hint, pen, stage1)]
    du = np.zeros(len(st), dtype=np.int8)
    sc = np.full(len(st), -1, dtype=np.int64)
    again = [int(j) for j in np.nonzero(st == -1)[0]]
    if again:
        part = part() if callable(part) else part
        voff = np.concatenate([[0], np.cumsum([int(it[0]) for it in part])])
        sub = _problem([part[j] for j in again], device)
        cut = lambda t: None if t is None else torch.cat([t[int(voff[j]):int(voff[j + 1])] for j in again])
        given = None if start is None else start.cpu().numpy()
        start2 = np.concatenate([model[voff[j]:voff[j + 1]] if co[j] >= 0 or given is None else given[voff[j]:voff[j + 1]] for j in again])
        r = [t.cpu().numpy() for t in sub.exact_nearest_split(cut(hint), cut(pen), torch.from_numpy(start2.astype(np.float32)).to(device),
                                                              depth=auto_depth(len(again), device), budget=budget, stats=True)[:8]]
        del sub
        off = 0
        for k, j in enumerate(again):
            n = int(voff[j + 1] - voff[j])
            st[j], co[j], du[j], sc[j] = r[0][k], r[1][k], r[6][k], r[7][k]
            wk[j] += r[3][k]
            model[voff[j]:voff[j + 1]] = r[2][off:off + n]
            off += n
    return st, co, model, wk, du, sc


def nearest_rounds_give(open_cubes, device):
    """split='rounds' of the nearest-model search: rounds_give's rule with k_exact_nearest_round's occupancy -- the smallest g with
    open_cubes * (1 + g) >= AUTO_CUBES_PER_WAVE cubes per resident wave, 0 once the frontier fills the GPU -- capped by
    NEAREST_ROUNDS_MAX_GIVE and by the 2^22 cubes of a frontier"""
    return _rounds_give(open_cubes, device, NEAREST_ROUNDS_WAVES_PER_SIMD, NEAREST_ROUNDS_MAX_GIVE)


def nearest_rounds_drop_spent(state, total):
    """The total budget of nearest_rounds, between two rounds: the cubes of every instance whose work has reached ``total`` (an int, or an
    int64 tensor of one value per instance on the state's device) leave the frontier of the NearestState; the instance's status stays -1
    and it keeps its cost and model.  Returns the number of instances that left."""
    return _drop_spent(state, total)[1]


def nearest_rounds(prob, part, budget, hint, pen, start, round_budget, give, rounds, device):
    """The nearest-model search of one problem in rounds (Problem.exact_nearest_round; ``part``: its loader items, or a callable that
    returns them, read only where an instance has more than 1023 variables; ``hint``, ``pen``, ``start``: tensors of V values, the last
    two or None): numpy (status, cost, model, work, rounds_used int32).  Every round runs every open cube for ``round_budget`` reads past
    its replay (None or 0: NEAREST_ROUND_BUDGET) under its instance's best cost so far and cuts the frontier it leaves again, ``give``
    levels per stopped cube (None: nearest_rounds_give of the open cubes, every round).  ``budget`` is the total of reads per instance
    over all rounds and cubes (0: the library's default budget): an instance whose work has reached it leaves the frontier with status
    -1 and keeps its cost and model.  ``rounds``: at most so many rounds (None: until no cube is open); instances that are still open
    then end with status -1 as well.  ``start`` is checked on the GPU and seeds the cost where it is a model.  An instance of more than
    1023 variables has no cube: it goes to the plain call, with ``budget``, and uses 0 rounds.  An instance with a penalty outside
    [0, 2^20] has status -3, cost 0 and a model of zeros, as in the plain call."""
    total = budget if budget > 0 else DEFAULT_BUDGET
    state = prob.exact_nearest_begin(hint, pen, start)
    done = 0
    while state.cubes and (rounds is None or done < rounds):
        prob.exact_nearest_round(state, round_budget or NEAREST_ROUND_BUDGET, nearest_rounds_give(state.cubes, device) if give is None else give)
        done += 1
        nearest_rounds_drop_spent(state, total)
    st, co, model = state.status.cpu().numpy(), state.cost.cpu().numpy(), state.model.cpu().numpy()
    wk, used = state.work.cpu().numpy(), state.rounds.cpu().numpy()
    co[st == -3] = 0
    wide = [int(j) for j in np.nonzero(st == -2)[0]]
    if wide:
        r = _on_their_own(part, wide, device, lambda sub, cut: sub.exact_nearest(cut(hint), cut(pen), budget), {2: model})
        st[wide], co[wide], wk[wide] = r[0], r[1], r[3]
    return st, co, model, wk, used


def nearest_model(items, hints, penalties=None, budget=0, device=None, max_edges=MAX_EDGES, split=None, start=None, depths=False):
    """The model of every loader item (as solve_items takes them) nearest to its hint, by branch and bound (pdp_exact_nearest; DESIGN.md
    §9.15).  Returns numpy (status int8 [N]: 1 cost is the minimum over the models, 0 the instance has no model, -1 the budget ran out and
    cost is that of the best model met, -1 if none was, -3 a penalty of the instance is outside [0, 2^20]; cost int64 [N]: the penalties
    of the variables where the model differs from the thresholded hint, summed; models: per instance a float32 0/1 array of n_i values,
    all 0 where cost is not >= 0 or status is -3; work int64 [N]).
    ``hints``: per instance an array of n_i values or None (> 0.5 true, every other value false, NaN included; None: all false), or None
    for all.  ``penalties``: per instance an integer array of n_i values or None (all 1), or None for all: the Hamming distance.
    ``split``: the search of every instance spread over 2^split waves that share the best cost found (pdp_exact_nearest_split; DESIGN.md
    §9.16; an int from 0 to 16), or 'auto': see nearest_split.  ``budget`` then applies to every cube.  A proved cost is the same minimum;
    which minimiser the model is and work depend on the timing of the cubes.  ``start``: per instance a model the caller already has
    (an array of n_i values, thresholded like a hint) or None, or None for all; the search of that instance starts below its distance,
    computed and checked on the GPU, and an array that is not a model is ignored.  Giving one turns on the split call (at depth 0 without
    ``split``).  ``depths``: also return depth_used int8 [N].  Without ``split`` and ``start`` the call is pdp_exact_nearest's.  The
    search in rounds is a call of its own, nearest_model_rounds: ``split='rounds'`` is refused here as it always was."""
    return _nearest_model(items, hints, penalties, budget, device, max_edges, _check_split(split), start, depths, None, None)


def nearest_model_rounds(items, hints, penalties=None, budget=0, device=None, max_edges=MAX_EDGES, start=None, round_budget=None, rounds=None,
                         depths=False):
    """nearest_model in rounds (nearest_rounds, pdp_exact_nearest_round): the same arguments and the same four outputs.
    Every round runs every open cube for ``round_budget`` reads past its replay (None: NEAREST_ROUND_BUDGET), at most ``rounds`` of them
    (None: until no cube is open); between two rounds the open part of every tree is cut again and the best cost of an instance is handed
    to all its cubes.  ``budget`` is the total of reads per instance over all rounds and cubes; a proved cost is nearest_model's minimum,
    every output is a function of the inputs, and which minimiser the model is depends on ``round_budget``.  ``start`` seeds the cost
    where it is a model.  ``depths``: also return the rounds every instance had a cube in (int32 [N])."""
    for name, x in (('round_budget', round_budget), ('rounds', rounds)):
        if x is not None and (isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1):
            raise ValueError("%s must be None or a positive integer, got %r" % (name, x))
    return _nearest_model(items, hints, penalties, budget, device, max_edges, 'rounds', start, depths, round_budget, rounds)


def _nearest_model(items, hints, penalties, budget, device, max_edges, split, start, depths, round_budget, rounds):
    "nearest_model and nearest_model_rounds (``split`` 'rounds'), segment by segment"
    by_rounds = isinstance(split, str) and split == 'rounds'
    native.require_gpu()
    for name, per in (('hints', hints), ('penalties', penalties), ('start', start)):
        if per is None:
            continue
        if len(per) != len(items):
            raise ValueError("%s: one entry per instance (%d), got %d" % (name, len(items), len(per)))
        for it, h in zip(items, per):
            if h is not None and np.asarray(h).size != int(it[0]):
                raise ValueError("%s: instance %r has %d variables, its %s %d values" % (name, it[5], int(it[0]), name, np.asarray(h).size))
    if penalties is not None:
        for it, q in zip(items, penalties):
            if q is not None and not np.issubdtype(np.asarray(q).dtype, np.integer):
                raise ValueError("penalties: instance %r has penalties of type %s, not integers" % (it[5], np.asarray(q).dtype))
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    status = np.ones(N, dtype=np.int8)
    cost = np.zeros(N, dtype=np.int64)
    work = np.zeros(N, dtype=np.int64)
    used = np.zeros(N, dtype=np.int32 if by_rounds else np.int8)
    models = [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        flat = [np.zeros(int(it[0]), dtype=np.float32) if hints is None or hints[i] is None else np.asarray(hints[i], dtype=np.float32).reshape(-1)
                for i, it in zip(seg, part)]
        # an instance without a start model passes its hint: the check pass has just rejected it, so it is ignored
        begin = None
        if start is not None:
            begin = [h if start[i] is None else np.asarray(start[i], dtype=np.float32).reshape(-1) for i, h in zip(seg, flat)]
        pens = None
        if penalties is not None:
            pens = [np.ones(int(it[0]), dtype=np.int64) if penalties[i] is None else np.asarray(penalties[i]).astype(np.int64).reshape(-1)
                    for i, it in zip(seg, part)]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere (and no problem to build: the layout needs an edge): without a clause the hint itself is the nearest
            # model, with an (empty) clause there is none
            for j, (i, it, h) in enumerate(zip(seg, part, flat)):
                if pens is not None and ((pens[j] < 0) | (pens[j] > MAX_PENALTY)).any():
                    status[i], models[i] = -3, np.zeros(int(it[0]), dtype=np.float32)
                elif int(it[1]) > 0:
                    status[i], cost[i], models[i] = 0, -1, np.zeros(int(it[0]), dtype=np.float32)
                else:
                    models[i] = (h > 0.5).astype(np.float32)
            continue
        with torch.cuda.device(device):
            prob = _problem(part, device)
            hint = torch.from_numpy(np.concatenate(flat)).to(device)
            pen = None
            if pens is not None:
                # a value that does not fit int32 is out of range either way: -1 stands for it
                allp = np.concatenate(pens)
                pen = torch.from_numpy(np.where((allp < 0) | (allp > MAX_PENALTY), -1, allp).astype(np.int32)).to(device)
            if by_rounds:
                first = None if begin is None else torch.from_numpy(np.concatenate(begin)).to(device)
                st, co, model, wk, du = nearest_rounds(prob, part, budget, hint, pen, first, round_budget, None, rounds, device)
            elif split is None and start is None:
                st, co, model, wk = [t.cpu().numpy() for t in prob.exact_nearest(hint, pen, budget)]
                du = np.zeros(len(part), dtype=np.int8)
            else:
                first = None if begin is None else torch.from_numpy(np.concatenate(begin)).to(device)
                st, co, model, wk, du, _ = nearest_split(prob, part, budget, hint, pen, first, 0 if split is None else split, device)
        del prob
        off = 0
        for j, (i, it) in enumerate(zip(seg, part)):
            n = int(it[0])
            status[i], cost[i], work[i], used[i] = st[j], co[j], wk[j], du[j]
            models[i] = model[off:off + n].copy()
            off += n
    return (status, cost, models, work, used) if depths else (status, cost, models, work)


def count_split(prob, part, budget, split, device):
    """The split count of one problem (``part``: its loader items, or a callable that returns them): numpy (status, count, true_count,
    work, depth_used).  ``split`` an int: one pdp_exact_count_split call at that depth.  'auto': a plain exact_count with
    AUTO_COUNT_STAGE1_BUDGET reads per instance (``budget`` if that is smaller), then the instances that ran out are counted again from the
    start -- a partial count cannot be resumed, so the first stage's is discarded -- as one split call on a problem of their own at
    auto_depth, with ``budget`` per cube; work is the sum of the two stages."""
    if split != 'auto':
        st, co, tc, wk, _, du = prob.exact_count_split(budget, depth=split, stats=True)[:6]
        return st.cpu().numpy(), co.cpu().numpy(), tc.cpu().numpy(), wk.cpu().numpy(), du.cpu().numpy()
    st, co, tc, wk = [t.cpu().numpy() for t in prob.exact_count(min(budget, AUTO_COUNT_STAGE1_BUDGET) if budget > 0 else AUTO_COUNT_STAGE1_BUDGET)]
    du = np.zeros(len(st), dtype=np.int8)
    again = [int(j) for j in np.nonzero(st == -1)[0]]
    if again:
        depth = auto_depth(len(again), device)
        r = _on_their_own(part, again, device, lambda sub, cut: sub.exact_count_split(budget, depth=depth, stats=True)[:6], {2: tc})
        st[again], co[again], du[again] = r[0], r[1], r[5]
        wk[again] += r[3]
    return st, co, tc, wk, du


def rounds_give(open_cubes, device):
    """split='rounds': the levels every stopped cube gives away so that ``open_cubes`` of them become AUTO_CUBES_PER_WAVE cubes per resident
    wave of k_exact_count_round -- the smallest g with open_cubes * (1 + g) >= that target, 0 once the frontier fills the GPU -- capped
    by ROUNDS_MAX_GIVE and by the 2^22 cubes of a frontier"""
    return _rounds_give(open_cubes, device, ROUNDS_WAVES_PER_SIMD, ROUNDS_MAX_GIVE)


def count_rounds(prob, part, budget, round_budget, give, rounds, device):
    """The count of one problem in rounds (Problem.exact_count_round; ``part`` is not read: a state is continued, nothing is counted
    twice): numpy (status, count, true_count, work, rounds_used int32).  Every round runs every open cube for ``round_budget`` reads past
    its replay (None or 0: ROUND_BUDGET) and cuts the frontier it leaves again, ``give`` levels per stopped cube (None: rounds_give of the
    open cubes, every round).  ``budget`` is the total of reads per instance over all rounds and cubes (0: the library's default budget):
    an instance whose work has reached it is not scheduled again and ends with status -1 and a lower bound.  ``rounds``: at most so many
    rounds (None: until no cube is open); instances that are still open then end with status -1 as well."""
    total = budget if budget > 0 else DEFAULT_BUDGET
    state = prob.exact_count_begin()
    ended = torch.zeros(prob.B, dtype=torch.bool, device=state.status.device)
    done = 0
    while state.cubes and (rounds is None or done < rounds):
        prob.exact_count_round(state, round_budget or ROUND_BUDGET, rounds_give(state.cubes, device) if give is None else give)
        done += 1
        ended |= _drop_spent(state, total)[0]                                     # out of reads: the totals stay as the lower bound they are
    status = torch.where(ended, torch.full_like(state.status, -1), state.status)
    return (status.cpu().numpy(), state.count.cpu().numpy(), state.true_count.cpu().numpy(), state.work.cpu().numpy(),
            state.rounds.cpu().numpy())


def count_models(items, budget=0, device=None, max_edges=MAX_EDGES, split=None, depths=False, round_budget=None, rounds=None):
    """Exact model counts of loader items (as solve_items takes them) by the counting search (pdp_exact_count).  Returns numpy (status int8
    [N]: 1 count is the number of models, -1 the budget ran out and it is a lower bound, -2 the instance has more than 1023 variables and
    was not searched; count float64 [N], over all n_i variables of an instance, unused ones included; marginals: per instance a float64
    array of n_i values, the share of the counted models in which the variable is true, or None where count is 0; work int64 [N]).
    count_is_exact says where count is an integer without rounding.
    ``split``: the count of every instance spread over 2^split waves (pdp_exact_count_split; an int from 0 to 16), or 'auto': see
    count_split.  Status, count and marginals are those of the call without ``split`` while count <= 2^53 and no cube runs out of
    ``budget``, which then applies to every cube; work is the sum over the cubes.  ``depths``: also return depth_used int8 [N].
    ``split='rounds'``: see count_rounds -- the count in rounds of ``round_budget`` reads per cube, at most ``rounds`` of them, the open
    part of every tree cut again between two rounds to fill the GPU.  ``budget`` is then the total of reads per instance; status, count
    and marginals are those of the plain call while count <= 2^53 and the total is not reached; ``depths``: the rounds used, int32 [N]."""
    by_rounds = isinstance(split, str) and split == 'rounds'
    if not by_rounds:
        split = _check_split(split)
        if round_budget is not None or rounds is not None:
            raise ValueError("round_budget and rounds belong to split='rounds'")
    else:
        for name, x in (('round_budget', round_budget), ('rounds', rounds)):
            if x is not None and (isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1):
                raise ValueError("%s must be None or a positive integer, got %r" % (name, x))
    native.require_gpu()
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    status = np.ones(N, dtype=np.int8)
    count = np.zeros(N, dtype=np.float64)
    work = np.zeros(N, dtype=np.int64)
    used = np.zeros(N, dtype=np.int32 if by_rounds else np.int8)
    marginals = [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere (and no problem to build: the layout needs an edge): without a clause every assignment is a model,
            # with an (empty) clause none is
            for i, it in zip(seg, part):
                n = int(it[0])
                if n > COUNT_MAX_N:
                    status[i] = -2
                elif int(it[1]) == 0:
                    count[i] = np.ldexp(1.0, n)
                    marginals[i] = np.full(n, 0.5, dtype=np.float64)
            continue
        with torch.cuda.device(device):
            prob = _problem(part, device)
            if split is None:
                st, co, tc, wk = [t.cpu().numpy() for t in prob.exact_count(budget)]
                du = np.zeros(len(part), dtype=np.int8)
            elif by_rounds:
                st, co, tc, wk, du = count_rounds(prob, part, budget, round_budget, None, rounds, device)
            else:
                st, co, tc, wk, du = count_split(prob, part, budget, split, device)
        del prob
        off = 0
        for j, (i, it) in enumerate(zip(seg, part)):
            n = int(it[0])
            status[i], count[i], work[i], used[i] = st[j], co[j], wk[j], du[j]
            if co[j] > 0:
                marginals[i] = tc[off:off + n] / co[j]
            off += n
    return (status, count, marginals, work, used) if depths else (status, count, marginals, work)


def mass_split(prob, part, weights, budget, split, device):
    """The split solution mass of one problem (``part``: its loader items, or a callable that returns them; ``weights``: the float32
    tensor of the problem's V weights on its device): numpy (status, mass, true_mass, open_mass, work, depth_used).  ``split`` an int: one
    pdp_exact_mass_split call at that depth.  'auto': a plain exact_mass with AUTO_MASS_STAGE1_BUDGET reads per instance (``budget`` if
    that is smaller), then the instances that ran out are weighed again from the start -- a partial search cannot be resumed, so the first
    stage's outputs are discarded -- as one split call on a problem of their own at auto_depth, with ``budget`` per cube; work is the sum
    of the two stages."""
    if split != 'auto':
        st, ma, tm, op, wk, _, du = prob.exact_mass_split(weights, budget, depth=split, stats=True)[:7]
        return st.cpu().numpy(), ma.cpu().numpy(), tm.cpu().numpy(), op.cpu().numpy(), wk.cpu().numpy(), du.cpu().numpy()
    stage1 = min(budget, AUTO_MASS_STAGE1_BUDGET) if budget > 0 else AUTO_MASS_STAGE1_BUDGET
    st, ma, tm, op, wk = [t.cpu().numpy() for t in prob.exact_mass(weights, stage1)]
    du = np.zeros(len(st), dtype=np.int8)
    again = [int(j) for j in np.nonzero(st == -1)[0]]
    if again:
        part = part() if callable(part) else part
        voff = np.concatenate([[0], np.cumsum([int(it[0]) for it in part])])
        sub = _problem([part[j] for j in again], device)
        w2 = torch.cat([weights[voff[j]:voff[j + 1]] for j in again]).contiguous()
        r = [t.cpu().numpy() for t in sub.exact_mass_split(w2, budget, depth=auto_depth(len(again), device), stats=True)[:7]]
        del sub
        off = 0
        for k, j in enumerate(again):
            n = int(voff[j + 1] - voff[j])
            st[j], ma[j], op[j], du[j] = r[0][k], r[1][k], r[3][k], r[6][k]
            wk[j] += r[4][k]
            tm[voff[j]:voff[j + 1]] = r[2][off:off + n]
            off += n
    return st, ma, tm, op, wk, du


def mass_logit_gradient(weights, posterior):
    """The gradient of -ln(mass) in the logits of a prediction, per instance ``weights - posterior`` (float64; zeros where the posterior is
    None, i.e. the mass is 0 and the loss has no finite gradient).  Z is multilinear in p, so dZ/dp_v = Z1 - Z0 (the masses with v fixed
    true / false, its own weight left out), and with p_v = sigmoid(logit_v): d(-ln Z)/d logit_v = -p_v (1 - p_v)(Z1 - Z0) / Z = p_v -
    p_v Z1 / Z = p_v - posterior_v.  With a posterior of status 1 this is the exact gradient of the likelihood loss; at status -1 it is
    the gradient of the lower bound's loss (the mass of the part of the tree visited)."""
    if len(weights) != len(posterior):
        raise ValueError("weights and posterior must hold one array per instance: %d and %d" % (len(weights), len(posterior)))
    out = []
    for i, (w, q) in enumerate(zip(weights, posterior)):
        w = np.asarray(w, dtype=np.float32).reshape(-1).astype(np.float64)
        if q is None:
            out.append(np.zeros(w.size, dtype=np.float64))
            continue
        q = np.asarray(q, dtype=np.float64).reshape(-1)
        if q.size != w.size:
            raise ValueError("posterior[%d] must have %d values (one per variable), got %d" % (i, w.size, q.size))
        out.append(w - q)
    return out


def solution_mass(items, weights, budget=0, device=None, max_edges=MAX_EDGES, split=None, depths=False):
    """The exact solution mass of soft predictions for loader items (pdp_exact_mass): with ``weights`` (per instance an
    array of n_i probabilities of the variables being true, taken as float32) rounded independently, how likely the result is a model.
    Returns numpy (status int8 [N]: 1 mass is that probability, -1 the budget ran out and it lies in [mass, mass + open_mass], -2 more
    than 1023 variables, -3 a weight is NaN or outside [0, 1], neither searched; mass float64 [N]; posterior: per instance a float64
    array of n_i values, P(variable true | the draw is a model) over the part of the tree visited, or None where mass is 0; open_mass
    float64 [N]; work int64 [N]).
    ``split``: the search of every instance spread over 2^split waves (pdp_exact_mass_split; an int from 0 to 16), or
    'auto': see mass_split.  ``budget`` then applies to every cube and work is the sum over the cubes; mass and posterior are those of
    the call without ``split`` up to the last bits (bit for bit where every product is exact).  ``depths``: also return depth_used int8
    [N]."""
    split = _check_split(split)
    native.require_gpu()
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    if len(weights) != N:
        raise ValueError("weights must hold one array per item: %d items, %d arrays" % (N, len(weights)))
    weights = [np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1)) for w in weights]
    for i, (it, w) in enumerate(zip(items, weights)):
        if w.size != int(it[0]):
            raise ValueError("weights[%d] must have %d values (one per variable), got %d" % (i, int(it[0]), w.size))
    status = np.ones(N, dtype=np.int8)
    mass = np.zeros(N, dtype=np.float64)
    open_mass = np.zeros(N, dtype=np.float64)
    work = np.zeros(N, dtype=np.int64)
    used = np.zeros(N, dtype=np.int8)
    posterior = [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere (and no problem to build: the layout needs an edge): without a clause every draw is a model and the
            # posterior is the prior, with an (empty) clause none is
            for i, it in zip(seg, part):
                w = weights[i]
                if int(it[0]) > COUNT_MAX_N:
                    status[i] = -2
                elif not bool(((w >= 0) & (w <= 1)).all()):
                    status[i] = -3
                elif int(it[1]) == 0:
                    mass[i] = 1.0
                    posterior[i] = w.astype(np.float64)
            continue
        with torch.cuda.device(device):
            prob = _problem(part, device)
            wt = torch.from_numpy(np.concatenate([weights[i] for i in seg])).to(device)
            if split is None:
                st, ma, tm, op, wk = [t.cpu().numpy() for t in prob.exact_mass(wt, budget)]
                du = np.zeros(len(part), dtype=np.int8)
            else:
                st, ma, tm, op, wk, du = mass_split(prob, part, wt, budget, split, device)
        del prob
        off = 0
        for j, (i, it) in enumerate(zip(seg, part)):
            n = int(it[0])
            status[i], mass[i], open_mass[i], work[i], used[i] = st[j], ma[j], op[j], wk[j], du[j]
            if ma[j] > 0:
                posterior[i] = tm[off:off + n] / ma[j]
            off += n
    return (status, mass, posterior, open_mass, work, used) if depths else (status, mass, posterior, open_mass, work)


def count_is_exact(status, count):
    "boolean array: the search was complete and count <= 2^53, so count and the per-variable counts are exact integers"
    return (np.asarray(status) == 1) & (np.asarray(count, dtype=np.float64) <= 2.0 ** 53)


def models_at(items, ranks, budget=0, device=None, max_edges=MAX_EDGES):
    """The models of given ranks in the counting search's own order (pdp_exact_models_at): rank r of an instance is its
    r-th model, r from 0, in the order count_models meets them, so ranks 0 .. count - 1 are all its models, each once, and the model of
    a rank depends on the instance and the rank alone.  ``ranks``: per instance an integer array in any order, each in 0 .. 2^53 - 1
    (None or empty: none).  Returns (status int8 [N]: 1 every rank of the instance is answered, -1 the budget ran out first, -2 more than
    1023 variables; count_seen float64 [N]: the count when the search ended, the model count if a rank >= it was asked; found: per
    instance an int8 array, 1 the row is that rank's model, 0 there is no such model, -1 not known; models: per instance a uint8 array
    [k_i, n_i], rows in the order of ``ranks``, zero where found != 1; work int64 [N])."""
    native.require_gpu()
    if len(ranks) != len(items):
        raise ValueError("ranks: one entry per instance (%d), got %d" % (len(items), len(ranks)))
    asked = []
    for it, r in zip(items, ranks):
        r = np.zeros(0, dtype=np.int64) if r is None else np.asarray(r)
        if r.size and (r.dtype.kind not in 'iu' or int(r.min()) < 0 or int(r.max()) >= MAX_RANK):
            raise ValueError("ranks: instance %r needs integers in 0 .. 2^53 - 1" % (it[5],))
        asked.append(r.astype(np.int64).reshape(-1))
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    status = np.ones(N, dtype=np.int8)
    seen = np.zeros(N, dtype=np.float64)
    work = np.zeros(N, dtype=np.int64)
    found, models = [None] * N, [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere (and no problem to build: the layout needs an edge): without a clause the search has one leaf with every
            # variable free, so rank r < 2^n is the binary digits of r; with an (empty) clause there is no model
            for i, it in zip(seg, part):
                n, r = int(it[0]), asked[i]
                found[i] = np.zeros(r.size, dtype=np.int8)
                models[i] = np.zeros((r.size, n), dtype=np.uint8)
                if n > COUNT_MAX_N:
                    status[i] = -2
                    found[i][:] = -1
                elif r.size and int(it[1]) == 0:
                    seen[i] = np.ldexp(1.0, n)
                    found[i][:] = r < seen[i]
                    bits = (r[:, None] >> np.minimum(np.arange(n), 63)[None, :]) & 1
                    models[i][:] = np.where(found[i][:, None] == 1, bits, 0)
            continue
        order = [np.argsort(asked[i], kind='stable') for i in seg]
        off = np.concatenate([[0], np.cumsum([asked[i].size for i in seg])]).astype(np.int64)
        flat = np.concatenate([asked[i][o] for i, o in zip(seg, order)]) if off[-1] else np.zeros(0, dtype=np.int64)
        with torch.cuda.device(device):
            prob = _problem(part, device)
            st, cs, fo, mo, wk = [t.cpu().numpy() for t in prob.exact_models_at(torch.from_numpy(flat).to(device),
                                                                                torch.from_numpy(off).to(device), budget)]
        del prob
        at = 0
        for j, (i, it, o) in enumerate(zip(seg, part, order)):
            n, k = int(it[0]), asked[i].size
            status[i], seen[i], work[i] = st[j], cs[j], wk[j]
            found[i] = np.empty(k, dtype=np.int8)
            found[i][o] = fo[off[j]:off[j + 1]]
            models[i] = np.empty((k, n), dtype=np.uint8)
            models[i][o] = mo[at:at + k * n].reshape(k, n)
            at += k * n
    return status, seen, found, models, work


def enumerate_models(items, limit, budget=0, device=None, max_edges=MAX_EDGES):
    """The first ``limit`` models of every instance in the counting search's order (models_at with ranks 0 .. limit - 1): (models: per
    instance a uint8 array [min(count, limit), n_i]; complete: boolean array, True where those are all the models of the instance --
    the search ran to its end within ``limit`` models and the budget)."""
    limit = int(limit)
    if limit < 0:
        raise ValueError("limit must be >= 0, got %d" % limit)
    # one rank more than asked for tells "exactly limit models" from "more"
    status, _, found, models, _ = models_at(items, [np.arange(limit + 1, dtype=np.int64)] * len(items), budget, device, max_edges)
    out = [m[:limit][f[:limit] == 1] for f, m in zip(found, models)]
    complete = np.array([st == 1 and f[limit] == 0 for st, f in zip(status, found)], dtype=bool)
    return out, complete


def sample_ranks(count, k, seed, index):
    "the k ranks sample_models draws for the instance at position ``index`` of its items: uniform on 0 .. count - 1, a function of (seed, index, count, k)"
    return np.random.Generator(np.random.Philox(key=[int(seed), int(index)])).integers(0, int(count), size=int(k))


def sample_models(items, k, seed=0, budget=0, counts=None, device=None, max_edges=MAX_EDGES):
    """k models of every instance drawn uniformly, with replacement, from ALL its models: uniform ranks below the exact count, then
    models_at.  ``counts``: an earlier count_models result for the same items (its first two entries, status and count, are read);
    None: count_models(items, budget) is run here.  Returns (samples, ranks): per instance a uint8 array [k, n_i] in draw order and the
    int64 ranks drawn -- or None for both where no uniform sample exists: the count is a lower bound or above 2^53 (count_is_exact is
    False), the instance has no model, or models_at ran out of budget on one of the ranks.  Instance i draws from
    np.random.Philox(key=[seed, i]), i its index in ``items``, so its sample does not depend on the other instances or the batch cut."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1, got %d" % k)
    if counts is None:
        counts = count_models(items, budget, device, max_edges)
    exact = count_is_exact(counts[0], counts[1]) & (np.asarray(counts[1]) > 0)
    ranks = [sample_ranks(counts[1][i], k, seed, i) if exact[i] else None for i in range(len(items))]
    _, _, found, models, _ = models_at(items, ranks, budget, device, max_edges)
    good = [r is not None and bool((f == 1).all()) for r, f in zip(ranks, found)]
    return [m if g else None for m, g in zip(models, good)], [r if g else None for r, g in zip(ranks, good)]


def backbone(items, budget=0, device=None, max_edges=MAX_EDGES, arena=0):
    """The backbone of every satisfiable instance: (status int8 [N], backbones).  backbones[i] is an int8 array of n_i values -- +1 the
    variable is true in every model, -1 false in every model, 0 free, 2 not decided within the budget -- and None when instance i is not
    satisfiable or its own search was undecided.  With M the model of the base search, variable v is in the backbone iff the instance is
    unsatisfiable under the single assumption v = not M[v].  One base solve_items(learn=True), then the n_i queries of every satisfiable
    instance as one solve_items(assume=...) call: each query is the instance's own item with a one-hot assumption array, thousands of
    small searches on the same clauses per launch."""
    status, models, _ = solve_items(items, budget=budget, device=device, max_edges=max_edges, learn=True, arena=arena)
    return status, backbone_of(items, status, models, budget=budget, device=device, max_edges=max_edges, arena=arena)


def backbone_of(items, status, models, budget=0, device=None, max_edges=MAX_EDGES, arena=0):
    """backbone()'s second result from answers already at hand: ``models[i]`` is a model of every instance with status[i] == 1 (any model
    gives the same backbone: a forced variable has one value in all of them)."""
    queries, assume, at = [], [], []
    for i in np.nonzero(np.asarray(status) == 1)[0]:
        for v in range(len(models[i])):
            a = np.zeros(len(models[i]), dtype=np.int8)
            a[v] = -1 if models[i][v] > 0.5 else 1
            queries.append(items[i])
            assume.append(a)
            at.append((int(i), v))
    out = [np.zeros(len(models[i]), dtype=np.int8) if status[i] == 1 else None for i in range(len(items))]
    if queries:
        answer = solve_items(queries, budget=budget, device=device, max_edges=max_edges, arena=arena, assume=assume)[0]
        for (i, v), q in zip(at, answer):
            out[i][v] = (1 if models[i][v] > 0.5 else -1) if q == 0 else (0 if q == 1 else 2)
    return out


def items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, batch_size):
    """The loader items of a batch's tensors (the loader's instance-contiguous layout, unreplicated): per instance (n, m, graph_map with its
    own 0-based ids, edge_feature, -1.0, [])."""
    gm = graph_map.detach().cpu().numpy().astype(np.int64).reshape(2, -1)
    ef = edge_feature.detach().cpu().numpy().reshape(-1).astype(np.float32)
    bvm = batch_variable_map.detach().cpu().numpy().astype(np.int64).reshape(-1)
    bfm = batch_function_map.detach().cpu().numpy().astype(np.int64).reshape(-1)
    v0 = np.concatenate([[0], np.cumsum(np.bincount(bvm, minlength=batch_size)[:batch_size])])
    f0 = np.concatenate([[0], np.cumsum(np.bincount(bfm, minlength=batch_size)[:batch_size])])
    e0 = np.concatenate([[0], np.cumsum(np.bincount(bfm[gm[1]], minlength=batch_size)[:batch_size])])
    return [(int(v0[i + 1] - v0[i]), int(f0[i + 1] - f0[i]),
             (gm[:, e0[i]:e0[i + 1]] - np.array([[v0[i]], [f0[i]]])).astype(np.int32), ef[e0[i]:e0[i + 1]].copy(), -1.0, []) for i in range(batch_size)]


def _label(s):
    return True if s == 1 else (False if s == 0 else None)


def label_clause_lists(instances, budget=0, device=None, max_edges=MAX_EDGES, learn=False, arena=0, certify=False, split=None,
                       round_budget=None, rounds=None):
    """The batched labeller: [(n, clauses), ...] (clauses: lists of signed 1-based ints) -> [True / False / None, ...].
    ``certify``: only checked answers become labels (solve_items); an answer that is not certified is None.  ``split``, ``round_budget``
    and ``rounds``: solve_items'."""
    out = solve_items([raw_item(n, clauses) for n, clauses in instances], budget=budget, device=device, max_edges=max_edges,
                      learn=learn, arena=arena, certify=certify, split=split, round_budget=round_budget, rounds=rounds)
    if certify:
        return [_label(int(s)) if v == 1 else None for s, v in zip(out[0], out[3])]
    return [_label(int(s)) for s in out[0]]


def is_sat(var_num, iclause_list, budget=0, learn=False, arena=0, certify=False, split=None, round_budget=None, rounds=None):
    """The reference's labelling hook (generator.py:15-17) for one instance: True, False, or None when the budget ran out.  ``split``
    (an int depth, 'auto' or 'rounds'): the one instance's search spread over the GPU (solve_items)."""
    return label_clause_lists([(var_num, iclause_list)], budget=budget, learn=learn, arena=arena, certify=certify, split=split,
                              round_budget=round_budget, rounds=rounds)[0]
