"""SAT / UNSAT labels from the batched complete solver on the GPU (pdp_exact_solve and pdp_exact_solve_hinted, include/pdp_hip.h; DESIGN.md "Complete solver").

PDP is incomplete: it finds assignments but never proves an instance unsatisfiable, so the reference leaves labelling to "your SAT solver
of choice" (src/pdp/generator.py:15-17).  This module fills that hook: ``label_clause_lists`` labels many instances in a few launches,
``is_sat`` has the reference hook's signature, ``solve_items`` works on loader items.  A label is True (satisfiable), False
(unsatisfiable) or None (undecided within the budget of clause-literal reads per instance; 0 = the library default, 2^32).
"""

import numpy as np
import torch

from pdp import native
from pdp.factorgraph import dataset

MAX_EDGES = 1 << 24          # edges per problem handed to the library


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


def solve_items(items, budget=0, device=None, max_edges=MAX_EDGES, hints=None, learn=False, arena=0):
    """Solve loader items ((n, m, graph_map, edge_feature, label, misc) tuples: dataset.instance_from_clauses, dataset.random_ksat_items,
    dataset.parse_line, raw_item).  Returns numpy (status int8 [N] in {1, 0, -1}, models: a float32 0/1 array of n_i values per instance,
    work int64 [N]).  Instances are packed into problems of at most ``max_edges`` edges; nothing couples two instances.
    ``hints``: per instance an array of n_i phase hints (> 0.5 true first, other finite values false first, NaN none) or None (no hints for
    that instance); the search is then pdp_exact_solve_hinted's (include/pdp_hip.h).
    ``learn``: the search with conflict clause learning (pdp_exact_solve_learn) and ``arena`` words per instance for its learned clauses
    (0: four per literal); same answers, far fewer reads on structured instances."""
    if arena and not learn:
        raise ValueError("arena belongs to the learning search: pass learn=True")
    native.require_gpu()
    if hints is not None:
        if len(hints) != len(items):
            raise ValueError("hints: one entry per instance (%d), got %d" % (len(items), len(hints)))
        for it, h in zip(items, hints):
            if h is not None and np.asarray(h).size != int(it[0]):
                raise ValueError("hints: instance %r has %d variables, its hints %d values" % (it[5], int(it[0]), np.asarray(h).size))
    device = torch.device('cuda:0') if device is None else torch.device(device)
    N = len(items)
    status = np.zeros(N, dtype=np.int8)
    work = np.zeros(N, dtype=np.int64)
    models = [None] * N
    for seg in _segments(items, max_edges):
        part = [items[i] for i in seg]
        if sum(int(it[2].shape[1]) for it in part) == 0:
            # no literal anywhere, so there is nothing to search (and no problem to build: the layout needs an edge): an instance without
            # clauses is satisfiable, one whose clauses are all empty is not
            for i, it in zip(seg, part):
                status[i] = 1 if int(it[1]) == 0 else 0
                models[i] = np.zeros(int(it[0]), dtype=np.float32)
                h = None if hints is None or hints[i] is None else np.asarray(hints[i], dtype=np.float32).reshape(-1)
                if status[i] == 1 and h is not None and not np.isnan(h).any():
                    models[i] = (h > 0.5).astype(np.float32)           # the check pass accepts a complete hint: no clause objects
            continue
        b = dataset.to_torch(dataset.collate_segment(part), device)
        with torch.cuda.device(device):
            prob = native.Problem(b['graph_map'], b['batch_variable_map'], b['batch_function_map'], b['edge_feature'], batch_size=len(part))
            hint = None
            if hints is not None:
                flat = [np.full(int(it[0]), np.nan, dtype=np.float32) if hints[i] is None else np.asarray(hints[i], dtype=np.float32).reshape(-1)
                        for i, it in zip(seg, part)]
                hint = torch.from_numpy(np.concatenate(flat)).to(device)
            st, model, wk = prob.exact_solve(budget, hints=hint, learn=learn, arena=arena)
            st, model, wk = st.cpu().numpy(), model.cpu().numpy(), wk.cpu().numpy()
        del prob
        off = 0
        for j, (i, it) in enumerate(zip(seg, part)):
            n = int(it[0])
            status[i], work[i] = st[j], wk[j]
            models[i] = model[off:off + n].copy()
            off += n
    return status, models, work


def _label(s):
    return True if s == 1 else (False if s == 0 else None)


def label_clause_lists(instances, budget=0, device=None, max_edges=MAX_EDGES, learn=False, arena=0):
    """The batched labeller: [(n, clauses), ...] (clauses: lists of signed 1-based ints) -> [True / False / None, ...]."""
    status, _, _ = solve_items([raw_item(n, clauses) for n, clauses in instances], budget=budget, device=device, max_edges=max_edges,
                                learn=learn, arena=arena)
    return [_label(int(s)) for s in status]


def is_sat(var_num, iclause_list, budget=0, learn=False, arena=0):
    """The reference's labelling hook (generator.py:15-17) for one instance: True, False, or None when the budget ran out."""
    return label_clause_lists([(var_num, iclause_list)], budget=budget, learn=learn, arena=arena)[0]
