"""Host side of the complete solver (pdp.exact, pdp_exact_solve): the labelled dataset generator, the dataset CLI and the converter's
--label flag, and the independent reference solvers the GPU tests compare against (a brute-force enumerator and a small DPLL, kept here
and never importing pdp.exact).  No GPU needed."""
import argparse
import os
import sys
import zlib

import numpy as np
import pytest

from helpers import REPO


# ---- independent reference solvers ------------------------------------------------------------------------------------------------
def brute_force(n, clauses):
    "satisfiable? by enumerating the 2^n assignments (bit v-1 of a = value of variable v), filtered clause by clause"
    a = np.arange(1 << n, dtype=np.int64)
    for c in clauses:
        if a.size == 0:
            break
        ok = np.zeros(a.size, dtype=bool)
        for l in c:
            bit = (a >> (abs(l) - 1)) & 1
            ok |= (bit == 1) if l > 0 else (bit == 0)
        a = a[ok]
    return bool(a.size)


def dpll(n, clauses):
    "satisfiable? by DPLL with unit propagation (branching on the most frequent variable of the shortest open clauses)"
    def simplify(cls, lit):
        out = []
        for c in cls:
            if lit in c:
                continue
            out.append([l for l in c if l != -lit])
        return out

    def solve(cls):
        while True:
            if any(len(c) == 0 for c in cls):
                return False
            if not cls:
                return True
            unit = next((c[0] for c in cls if len(set(c)) == 1), None)
            if unit is None:
                break
            cls = simplify(cls, unit)
        w = min(len(set(c)) for c in cls)
        count = {}
        for c in cls:
            if len(set(c)) == w:
                for l in set(c):
                    count[l] = count.get(l, 0) + 1
        lit = max(count, key=lambda l: (count[l] + count.get(-l, 0), -abs(l), l > 0))
        return solve(simplify(cls, lit)) or solve(simplify(cls, -lit))

    # a tautological clause is always satisfied: drop it before the search
    return solve([list(c) for c in clauses if not any(-l in c for l in c)])


def pigeonhole(holes):
    "PHP(holes + 1, holes): variable p * holes + h + 1 = pigeon p sits in hole h; unsatisfiable"
    pigeons = holes + 1
    var = lambda p, h: p * holes + h + 1  # noqa: E731
    clauses = [[var(p, h) for h in range(holes)] for p in range(pigeons)]
    for h in range(holes):
        for p in range(pigeons):
            for q in range(p + 1, pigeons):
                clauses.append([-var(p, h), -var(q, h)])
    return pigeons * holes, clauses


HAND_MADE = [
    (3, [], True),                                    # no clauses
    (2, [[]], False),                                 # an empty clause
    (1, [[1], [-1]], False),                          # contradicting units
    (1, [[1, -1]], True),                             # tautology
    (2, [[1, 1], [-1, 2], [-2, -2]], False),          # repeated literals
    (2, [[1, 2], [-1, 2], [1, -2], [-1, -2]], False),
    (3, [[1, 2], [-1, 2], [1, -2]], True),            # variable 3 never occurs
    (5, [[1], [-1, 2], [-2, 3], [-3, 4], [-4, 5], [-5]], False),
    (4, [[1, 2, 3, 4]] + [[-1, -2], [-3, -4]], True),
    pigeonhole(2) + (False,),
    pigeonhole(3) + (False,),
]


@pytest.mark.parametrize('case', range(len(HAND_MADE)))
def test_reference_solvers_on_hand_made_cases(case):
    n, clauses, want = HAND_MADE[case]
    assert brute_force(n, clauses) == want
    assert dpll(n, clauses) == want


def test_reference_solvers_agree_on_random_instances():
    rng = np.random.RandomState(11)
    sat = 0
    for _ in range(300):
        n = int(rng.randint(1, 9))
        m = int(rng.randint(0, 5 * n + 1))
        clauses = [[int(v) * int(s) for v, s in zip(rng.randint(1, n + 1, size=k), rng.choice([-1, 1], size=k))]
                   for k in rng.randint(0, 4, size=m)]
        want = brute_force(n, clauses)
        sat += want
        assert dpll(n, clauses) == want, (n, clauses)
    assert 20 < sat < 280                              # both answers occur


# ---- the labelled dataset generator --------------------------------------------------------------------------------------------------
def fake_labeller(instances):
    "deterministic, draws no random numbers: True / False / None from a hash of the clause list"
    return [(True, False, None)[zlib.crc32(repr((n, c)).encode()) % 3] for n, c in instances]


def sequential_dataset(g, size, dimacs_dir, json_dir, name, sat_only, labeller):
    "the one-candidate-at-a-time run the batched generator must reproduce"
    os.makedirs(dimacs_dir, exist_ok=True)
    os.makedirs(json_dir, exist_ok=True)
    for j in range(g._alpha_resolution):
        postfix = '_%d_%s_%s' % (j, g._alpha, g._alpha + g._alpha_inc)
        os.makedirs(os.path.join(dimacs_dir, name) + postfix, exist_ok=True)
        with open(os.path.join(json_dir, name) + postfix + '.json', 'w') as f:
            for i in range(size):
                found = False
                for _ in range(50):
                    n, m, gm, ef, _, _, clause_list = g.generate_complete()
                    label = labeller([(n, clause_list)])[0]
                    if label is not None and (not sat_only or label):
                        found = True
                        break
                if found:
                    f.write(str(g._to_json(n, m, gm, ef, label)).replace("'", '"') + '\n')
                    with open(os.path.join(os.path.join(dimacs_dir, name) + postfix, 'dimacs_%d_sat=%s.DIMACS' % (i, label)), 'w') as h:
                        h.write(g._to_dimacs(n, m, clause_list) + '\n')
        g._alpha += g._alpha_inc


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def rng_state():
    s = np.random.get_state()
    return (s[0], s[1].tobytes(), s[2], s[3], s[4])


def _uniform():
    from pdp.cnf_generators import UniformCNFGenerator
    return UniformCNFGenerator(8, 14, 2, 4, 2.0, 9.0, alpha_resolution=3)


@pytest.mark.parametrize('sat_only', [True, False])
@pytest.mark.parametrize('label_batch', [None, 1, 7])
def test_generate_dataset_batched_labels_equal_sequential(tmp_path, sat_only, label_batch):
    np.random.seed(21)
    _uniform().generate_dataset(6, str(tmp_path / 'bd'), str(tmp_path / 'bj'), 'u', sat_only=sat_only, labeller=fake_labeller,
                                label_batch=label_batch)
    after_batched = rng_state()
    np.random.seed(21)
    sequential_dataset(_uniform(), 6, str(tmp_path / 'sd'), str(tmp_path / 'sj'), 'u', sat_only, fake_labeller)
    assert rng_state() == after_batched
    assert tree(str(tmp_path / 'bd')) == tree(str(tmp_path / 'sd'))
    assert tree(str(tmp_path / 'bj')) == tree(str(tmp_path / 'sj'))
    lines = [l for v in tree(str(tmp_path / 'bj')).values() for l in v.decode().split('\n') if l.strip()]
    assert lines and all(l.endswith(', 1]') or (not sat_only and l.endswith(', 0]')) for l in lines)
    names = [k for k in tree(str(tmp_path / 'bd'))]
    assert all('sat=True' in k for k in names) if sat_only else any('sat=False' in k for k in names)


def test_generate_dataset_modular_batched_labels_equal_sequential(tmp_path):
    from pdp.cnf_generators import ModularCNFGenerator
    mk = lambda: ModularCNFGenerator(3, 20, 30, 0.3, 0.9, 3, 6, 2.0, 6.0, alpha_resolution=2)  # noqa: E731
    np.random.seed(5)
    mk().generate_dataset(4, str(tmp_path / 'bd'), str(tmp_path / 'bj'), 'm', sat_only=True, labeller=fake_labeller)
    after = rng_state()
    np.random.seed(5)
    sequential_dataset(mk(), 4, str(tmp_path / 'sd'), str(tmp_path / 'sj'), 'm', True, fake_labeller)
    assert rng_state() == after
    assert tree(str(tmp_path / 'bd')) == tree(str(tmp_path / 'sd')) and tree(str(tmp_path / 'bj')) == tree(str(tmp_path / 'sj'))


@pytest.mark.parametrize('sat_only', [True, False])
def test_generate_dataset_without_labeller_is_the_stub_run(tmp_path, sat_only):
    "labeller=None: the stub's labels (always False), byte for byte the one-at-a-time run with a labeller that says False"
    np.random.seed(3)
    _uniform().generate_dataset(4, str(tmp_path / 'bd'), str(tmp_path / 'bj'), 'u', sat_only=sat_only)
    after = rng_state()
    np.random.seed(3)
    sequential_dataset(_uniform(), 4, str(tmp_path / 'sd'), str(tmp_path / 'sj'), 'u', sat_only, lambda inst: [False] * len(inst))
    assert rng_state() == after
    assert tree(str(tmp_path / 'bd')) == tree(str(tmp_path / 'sd')) and tree(str(tmp_path / 'bj')) == tree(str(tmp_path / 'sj'))


# ---- the two command lines -----------------------------------------------------------------------------------------------------------------
def test_generator_cli_flags():
    from pdp import generator
    a = generator.cli_parser().parse_args(['o', 'j', 'name', '12', 'modular', '--min_n', '10', '--max_n', '20', '--min_k', '4', '--res', '3',
                                           '--min_a', '1.5', '-s', '--label', 'none', '--budget', '77'])
    assert (a.out_dir, a.out_json, a.name, a.size, a.method) == ('o', 'j', 'name', 12, 'modular')
    assert (a.min_n, a.max_n, a.min_k, a.res, a.min_a, a.sat_only, a.label, a.budget) == (10, 20, 4, 3, 1.5, True, 'none', 77)
    d = generator.cli_parser().parse_args(['o', 'j', 'n', '1', 'uniform'])
    assert (d.min_n, d.max_n, d.min_c, d.max_c, d.min_q, d.max_q, d.min_k, d.max_k, d.min_a, d.max_a, d.res, d.sat_only) == \
        (40, 40, 10, 40, 0.3, 0.9, 3, 5, 2, 10, 5, False)
    assert d.label == 'exact' and d.budget == 0
    with pytest.raises(SystemExit):
        generator.cli_parser().parse_args(['o', 'j', 'n', '1', 'uniform', '--label', 'maybe'])
    assert isinstance(generator.make_generator('modular', a), generator.ModularCNFGenerator)
    assert isinstance(generator.make_generator('v-modular', a), generator.VariableModularCNFGenerator)
    assert isinstance(generator.make_generator('uniform', a), generator.UniformCNFGenerator)


@pytest.mark.parametrize('sat_only', [True, False])
def test_generator_cli_label_none_is_the_stub_output(tmp_path, sat_only):
    from pdp import generator
    from pdp.cnf_generators import UniformCNFGenerator
    np.random.seed(9)
    generator.main([str(tmp_path / 'cd'), str(tmp_path / 'cj'), 'x', '3', 'uniform', '--min_n', '10', '--max_n', '12', '--res', '2',
                    '--label', 'none'] + (['-s'] if sat_only else []))
    after = rng_state()
    np.random.seed(9)
    UniformCNFGenerator(10, 12, 3, 5, 2, 10, alpha_resolution=2).generate_dataset(3, str(tmp_path / 'gd'), str(tmp_path / 'gj'), 'x', sat_only)
    assert rng_state() == after
    assert tree(str(tmp_path / 'cd')) == tree(str(tmp_path / 'gd')) and tree(str(tmp_path / 'cj')) == tree(str(tmp_path / 'gj'))
    assert len(tree(str(tmp_path / 'cd'))) == (0 if sat_only else 6)


def test_converter_label_flag():
    sys.path.insert(0, os.path.join(REPO, 'pdp-solver_amd'))
    import dimacs2json
    p = dimacs2json.cli_parser()
    a = p.parse_args(['in', 'out', '--label', 'exact', '--budget', '9', '-p'])
    assert (a.in_dir, a.out_file, a.label, a.budget, a.positive, a.simplify) == ('in', 'out', 'exact', 9, True, False)
    d = p.parse_args(['in', 'out'])
    assert d.label == 'name' and d.budget == 0
    with pytest.raises(SystemExit):
        p.parse_args(['in', 'out', '--label', 'guess'])


def test_converter_without_label_flag_unchanged(tmp_path):
    "no --label: the lines of today's converter (tests/golden/cli_dimacs20.converted.jsonl)"
    import subprocess
    out = tmp_path / 'c.jsonl'
    subprocess.check_call([sys.executable, os.path.join(REPO, 'pdp-solver_amd', 'dimacs2json.py'), os.path.join(REPO, 'tests', 'golden', 'dimacs20'),
                           str(out)])
    got = sorted(l for l in out.read_text().split('\n') if l.strip())
    ref = sorted(l for l in open(os.path.join(REPO, 'tests', 'golden', 'cli_dimacs20.converted.jsonl')).read().split('\n') if l.strip())
    assert got == ref
