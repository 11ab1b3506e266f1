#!/usr/bin/env python3
"""DIMACS -> compact JSON converter (drop-in for the reference's src/dimacs2json.py).

Output lines are byte-identical to the reference's for valid input (``[[n, m], [signed vars], [clause ids], label,
[file name]]``, reference: dimacs2json.py:85-91,111,125) including its conventions: the last occurrence of a
variable inside a clause wins, empty clauses and unused variables are dropped, literals are clause-major with
ascending variable index, the label is the last digit of the file stem (directory mode, :105) or the character
8 from the end of the path (file mode, :118-122).  The parser streams clauses into sparse rows instead of the
reference's dense [clauses x variables] matrix (native single-pass parser, csrc/pdp_dimacs.hip), so big instances do
not need O(n*m) memory.  ``-s`` removes subsumed clauses in the reference's two passes (dimacs2json.py:60-83) through an inverted
literal index instead of its dense [clauses x clauses] product.
"""

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from pdp import generator  # noqa: E402


def parse_dimacs(path):
    """Pure-Python statement of the parsing rules: (declared variable count, list of clauses as lists of signed ints).
    The converter itself uses the native parser; the tests check the two against each other."""
    n = 0
    clauses = []
    with open(path, 'r') as f:
        for line in f:
            tok = line.split()
            if not tok or tok[0] == 'c' or tok[0] == '%':
                continue
            if tok[0] == 'p':
                n = int(tok[2])
                continue
            lits = []
            for t in tok:
                v = int(t)
                if v == 0:
                    break
                lits.append(v)
            clauses.append(lits)
    return n, clauses


def remove_subsumed(signed_vars, clause_ids):
    """The reference's ``_propagate_constraints`` (dimacs2json.py:60-83) on the compact edge list: pass 1 drops every clause that contains
    all literals of a LATER clause (equal clauses: the earlier one goes), pass 2 drops, among the survivors, every clause that contains
    all literals of an EARLIER one.  Variables keep their numbers (the reference compacts them before this step only).  Returns
    (signed_vars, clause_ids) with the surviving clauses renumbered 1..m' in order."""
    import numpy as np
    sv = np.asarray(signed_vars, dtype=np.int64); ci = np.asarray(clause_ids, dtype=np.int64)
    m = int(ci.max()) if ci.size else 0
    bounds = np.searchsorted(ci, np.arange(1, m + 2))
    clauses = [sv[bounds[i]:bounds[i + 1]].tolist() for i in range(m)]

    def survivors(cls, drop_superset_of_later):
        index = {}
        for i, c in enumerate(cls):
            for lit in c:
                index.setdefault(lit, []).append(i)
        keep = [True] * len(cls)
        for i, c in enumerate(cls):                        # clause i as the (candidate) subset
            if not c:
                continue
            lists = sorted((index[lit] for lit in c), key=len)
            common = set(lists[0])
            for lst in lists[1:]:
                common.intersection_update(lst)
                if not common:
                    break
            for j in common:                               # clause j contains every literal of clause i
                if drop_superset_of_later and j < i:
                    keep[j] = False
                if not drop_superset_of_later and j > i:
                    keep[j] = False
        return [c for c, k in zip(cls, keep) if k]

    if len(clauses) >= 2:
        clauses = survivors(clauses, True)
    if len(clauses) >= 2:
        clauses = survivors(clauses, False)
    out_sv = [lit for c in clauses for lit in c]
    out_ci = [i + 1 for i, c in enumerate(clauses) for _ in c]
    return np.asarray(out_sv, dtype=np.int32), np.asarray(out_ci, dtype=np.int32)


def compact_instance(path, propagate=False):
    "(var_num, clause_num, signed_vars, clause_ids) of one output line, read by the native parser of libpdp_hip.so (pdp_dimacs_open)"
    from pdp import native
    var_num, clause_num, signed_vars, clause_ids = native.dimacs_parse(path)
    if propagate:
        signed_vars, clause_ids = remove_subsumed(signed_vars, clause_ids)
        clause_num = int(clause_ids.max()) if clause_ids.size else 0
    return var_num, clause_num, signed_vars, clause_ids


def json_line(path, label, propagate=False):
    "One output line; the text is read by the native parser of libpdp_hip.so (pdp_dimacs_open, include/pdp_hip.h)."
    var_num, clause_num, signed_vars, clause_ids = compact_instance(path, propagate)
    return generator.format_json_line(var_num, clause_num, signed_vars, clause_ids, label=label, name=os.path.split(path)[1])


def exact_labels(instances, budget=0, learn=False, certify=False, cores=False):
    """Labels of compact instances ((var_num, clause_num, signed_vars, clause_ids) as written to the lines) from the complete GPU solver
    (pdp.exact), all instances in a few launches: 1.0 satisfiable, 0.0 unsatisfiable, -1 undecided within the budget (the converter's
    "no label" value).  ``learn``: the search with conflict clause learning (the same labels).  ``certify``: (labels, proofs) from the
    certified search (exact.solve_items): an answer that is not certified is labelled -1, and proofs holds the DRAT lines of every
    unsatisfiable instance (None for the others).  ``cores`` (with certify): (labels, proofs, cores) from the backward check -- proofs holds
    the lemmas the refutation needs only, cores the 0-based indices of the clauses it rests on (None for the others)."""
    import numpy as np
    from pdp import exact
    items = []
    for var_num, clause_num, signed_vars, clause_ids in instances:
        sv, ci = np.asarray(signed_vars, dtype=np.int64), np.asarray(clause_ids, dtype=np.int64)
        graph_map = np.stack((np.abs(sv) - 1, ci - 1)).astype(np.int32).reshape(2, -1)
        items.append((int(var_num), int(clause_num), graph_map, np.sign(sv).astype(np.float32), -1.0, []))
    if certify:
        out = exact.solve_items(items, budget=budget, certify=True, proofs=True, cores=cores)
        status, verdict, lemmas = out[0], out[3], out[4]
        labels = [(1.0 if s == 1 else 0.0) if s != -1 and v == 1 else -1 for s, v in zip(status, verdict)]
        proofs = [exact.drat_lines(l) if lab == 0.0 else None for lab, l in zip(labels, lemmas)]
        return (labels, proofs, [c if lab == 0.0 else None for lab, c in zip(labels, out[5])]) if cores else (labels, proofs)
    status, _, _ = exact.solve_items(items, budget=budget, learn=learn)
    return [1.0 if s == 1 else (0.0 if s == 0 else -1) for s in status]


def core_cnf_lines(instance, core):
    """The core of a compact instance ((var_num, clause_num, signed_vars, clause_ids) as written to its line; core: 0-based clause indices)
    as DIMACS text, with the variable numbers of that line -- the ones the lemmas of its .drat use."""
    var_num, _, signed_vars, clause_ids = instance
    rows = {}
    for l, c in zip(signed_vars, clause_ids):
        rows.setdefault(int(c) - 1, []).append(int(l))
    return ['p cnf %d %d' % (int(var_num), len(core))] + [' '.join([str(l) for l in rows.get(int(c), [])] + ['0']) for c in core]


def convert_directory(dimacs_dir, output_file, propagate=False, only_positive=False, label='name', budget=0, proof_dir=None, core=False):
    """label 'name': the reference's rule (the last digit of the file stem, else -1); 'exact': the complete solver's answer for the
    instance the line holds (exact_labels), 'exact-learn': the same from the learning search, 'exact-certified': the same with every answer
    checked on the GPU (an answer that is not certified is labelled -1) and, with ``proof_dir``, one <file name>.drat per unsatisfiable
    instance there.  ``core`` (with 'exact-certified' and ``proof_dir``): the unsatisfiable answers are certified by the backward check;
    <file name>.drat holds only the lemmas the refutation needs and a new <file name>.core.cnf the clauses it rests on, in the variable
    numbering of the instance's line, so that the .drat is a proof of the .core.cnf alone.  Every other byte of a line is the same either way."""
    if core and (label != 'exact-certified' or not proof_dir):
        raise ValueError("core needs label 'exact-certified' and a proof_dir to write to")
    file_list = [os.path.join(dimacs_dir, f) for f in os.listdir(dimacs_dir) if os.path.isfile(os.path.join(dimacs_dir, f))]
    if label in ('exact', 'exact-learn', 'exact-certified'):
        paths = [p for p in file_list if os.path.splitext(p)[1].lower() in ('.dimacs', '.cnf')]
        instances = [compact_instance(p, propagate) for p in paths]
        labels = []
        if instances and label == 'exact-certified':
            out = exact_labels(instances, budget, certify=True, cores=core)
            labels, proofs, cores = out if core else out + (None,)
            if proof_dir:
                os.makedirs(proof_dir, exist_ok=True)
                for k, (path, lines) in enumerate(zip(paths, proofs)):
                    if lines is not None:
                        with open(os.path.join(proof_dir, os.path.split(path)[1] + '.drat'), 'w') as g:
                            g.write('\n'.join(lines) + '\n')
                        if core:
                            with open(os.path.join(proof_dir, os.path.split(path)[1] + '.core.cnf'), 'w') as g:
                                g.write('\n'.join(core_cnf_lines(instances[k], cores[k])) + '\n')
        elif instances:
            labels = exact_labels(instances, budget, learn=label == 'exact-learn')
        with open(output_file, 'w') as f:
            for path, inst, lab in zip(paths, instances, labels):
                if only_positive and lab == 0:
                    continue
                f.write(generator.format_json_line(*inst, label=lab, name=os.path.split(path)[1]) + '\n')
        return
    with open(output_file, 'w') as f:
        for path in file_list:
            name, ext = os.path.splitext(path)
            if ext.lower() not in ('.dimacs', '.cnf'):
                continue
            label = float(name[-1]) if name[-1].isdigit() else -1
            if only_positive and label == 0:
                continue
            f.write(json_line(path, label, propagate) + '\n')


def convert_file(file_name, output_file, propagate=False):
    if len(file_name) < 8:
        label = -1
    else:
        c = file_name[-8]
        label = float(c) if c.isdigit() else -1
    with open(output_file, 'w') as f:
        f.write(json_line(file_name, label, propagate) + '\n')


def cli_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('in_dir', action='store', type=str)
    parser.add_argument('out_file', action='store', type=str)
    parser.add_argument('-s', '--simplify', help='Propagate binary constraints', required=False, action='store_true', default=False)
    parser.add_argument('-p', '--positive', help='Output only positive examples', required=False, action='store_true', default=False)
    parser.add_argument('--label', choices=('name', 'exact', 'exact-learn', 'exact-certified'), default='name',
                        help="name: the last digit of the file name (the reference's rule); exact: solve every instance on the GPU; "
                             "exact-learn: the same with conflict clause learning; exact-certified: the learning search with every answer checked "
                             "on the GPU (pdp_exact_check), an answer that is not certified is labelled -1")
    parser.add_argument('--proof-dir', dest='proof_dir', default=None,
                        help="with --label exact-certified: write <file name>.drat (the learned clauses as DRAT text) per unsatisfiable instance here")
    parser.add_argument('--core', action='store_true', default=False,
                        help="with --label exact-certified --proof-dir: certify the unsatisfiable answers by the backward check (pdp_exact_trim); "
                             "<file name>.drat holds only the lemmas the refutation needs and <file name>.core.cnf the clauses it rests on, in the "
                             "compact variable numbering of the written line (unused variable ids of the input file are dropped), which the .drat uses")
    parser.add_argument('--budget', type=int, default=0, help="clause-literal reads per instance for --label exact / exact-learn (0: the library default)")
    return parser


if __name__ == '__main__':
    parser = cli_parser()
    args = vars(parser.parse_args())
    if args['core'] and (args['label'] != 'exact-certified' or not args['proof_dir']):
        parser.error("--core writes the core next to the proof: give --label exact-certified and --proof-dir as well")
    convert_directory(args['in_dir'], args['out_file'], args['simplify'], args['positive'], args['label'], args['budget'], args['proof_dir'], args['core'])
