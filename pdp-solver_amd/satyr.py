#!/usr/bin/env python3
"""Run a PDP solver against a test set on the MI355X (drop-in for the reference's src/satyr.py).

Same positionals, flags, YAML keys and output format as the reference CLI (reference: satyr.py:45-109).
Additions: ``--rng {torch,philox}`` (torch = the reference's CPU random stream, bit-compatible results for the
same ``-s`` seed; philox = on-device counters, fastest), ``--stepwise`` (disable the one-launch persistent loop) and ``--isolated``
(every instance on its own instead of the reference's batch-wide couplings), and ``--complete`` / ``--complete-budget N``: every instance
is then decided by the batched exact search with the model's assignment as its phase hints (pdp_exact_solve_hinted), and a row gains
"complete" (1 satisfiable, 0 unsatisfiable, -1 undecided within the budget), "pdp_solved" and "work"; ``--complete-learn`` gives that search
conflict clause learning (pdp_exact_solve_learn); ``--complete-certify`` (implies ``--complete-learn``) has every answer checked on the GPU -- a
model against the clauses, an "unsatisfiable" by a forward check of the learned clauses as a proof (pdp_exact_check) -- and a row gains
"certified" (1 checked, -1 undecided); ``--complete-core`` (with ``--complete-certify``) judges an "unsatisfiable" by the backward check
(pdp_exact_trim) and such a row gains "core", the 0-based indices of the clauses its refutation rests on; ``--complete-backbone`` (with
``--complete``) gives a satisfiable row "backbone", the signed 1-based literals that hold in every model of the instance (one query of
the search under assumptions per variable, pdp_exact_solve_learn_assume), and "backbone_unknown" when queries ran out of budget;
``--complete-min-unsat`` (with ``--complete``) gives every row that is not satisfiable "min_unsat", the fewest clauses any assignment leaves
unsatisfied (pdp_exact_min_unsat, branch and bound from the model's assignment), "min_unsat_proved" (1 / 0: the budget ran out and it is
an upper bound), "min_unsat_solution" and "min_unsat_work"; ``--complete-count`` (with ``--complete``) gives every satisfiable row "model_count",
the exact number of its models (pdp_exact_count), "model_count_log2", "model_count_proved" (1 / 0: the budget ran out and it is a lower bound),
"marginals" (per variable, the share of the models in which it is true), "marginal_gap" (the mean distance of the model's soft prediction
from them) and "count_work"; ``--complete-split N`` (with ``--complete``, not with ``--complete-learn`` or ``--complete-certify``) spreads the
search of every instance over 2^N waves (pdp_exact_solve_split; -1: a plain first stage, then a depth chosen from the number of
undecided instances): the same "complete" and solution, "work" summed over the cubes, and "split_depth" on the rows searched at a depth
above 0; ``--complete-rounds N`` (with ``--complete``, not with ``--complete-split``, ``--complete-learn`` or ``--complete-certify``) runs
that search in rounds of 2^N reads per cube (pdp_exact_solve_round; -1: the default) and cuts the open part of every tree again between
two rounds: the same "complete", a model of the instance as the solution, ``--complete-budget`` as the total per row, "work" summed over
rounds and cubes, and "complete_rounds" on every row searched this way; ``--complete-count-split N`` (with ``--complete-count``) does the same for the count (pdp_exact_count_split; -1: a plain first count,
then the instances that ran out once more at a depth chosen from their number): the same counts and marginals, "count_work" summed over
the cubes, and "count_split_depth" on the rows counted at a depth above 0; ``--complete-count-rounds N`` (with ``--complete-count``, not
with ``--complete-count-split``) counts in rounds of 2^N reads per cube (pdp_exact_count_round; -1: the default) and cuts the open part of
every tree again between two rounds: the same counts and marginals, ``--complete-budget`` as the total per row, "count_work" summed over
rounds and cubes, and "count_rounds" on every counted row; ``--complete-min-unsat-split N`` (with ``--complete-min-unsat``)
spreads that branch and bound over 2^N waves per row that share the best cost found (pdp_exact_min_unsat_split; -1: a plain first stage,
then the rows left unproved once more from the cost reached): "min_unsat" and "min_unsat_proved" mean the same, "min_unsat_work" is summed
over the cubes, and "min_unsat_split_depth" appears on the rows searched at a depth above 0; ``--complete-sample K`` (with ``--complete-count``) gives every row
whose count is proved and exact "samples", K models in the format of "solution" drawn uniformly from all its models (pdp_exact_models_at at
uniform ranks below the count, seeded by ``-s``), and "sample_ranks", the ranks drawn; every other row is unchanged;
``--complete-mass`` (with ``--complete``, independent of ``--complete-count``) gives every satisfiable row "solution_mass", the probability
that rounding every variable independently with the model's soft prediction gives a model of the instance (pdp_exact_mass),
"solution_mass_log2", "solution_mass_open" (the mass of the part of the tree not visited within the budget: the true value lies in
[solution_mass, solution_mass + solution_mass_open]), "solution_mass_proved" (1 / 0), "posterior" (per variable, P(true | the draw is a
model); left out where the mass is 0) and "mass_work".  After Walk-SAT (``-w`` above 0) the prediction is 0/1, the mass is 1 or 0 and
costs one descent: the flag is meant for runs whose prediction is soft (``-w 0``); ``--complete-mass-split N`` (with ``--complete-mass``)
spreads that search over 2^N waves per row (pdp_exact_mass_split; -1: a plain first stage, then the rows that ran out once more at a depth
chosen from their number): the budget applies per cube, so a bracket is tightened by 2^N times the reads, "mass_work" is summed over the
cubes, and "mass_split_depth" appears on the rows weighed at a depth above 0; ``--complete-nearest`` (with ``--complete``) gives every
satisfiable row "nearest", the fewest variables in which a model of the instance differs from the model's own assignment
(pdp_exact_nearest, branch and bound from that assignment; left out where no model was met within the budget), "nearest_proved" (1 / 0: the
budget ran out and it is an upper bound), "nearest_solution" (that model) and "nearest_work"; a row PDP solved gets "nearest" 0; ``--complete-nearest-split N`` (with
``--complete-nearest``) spreads that branch and bound over 2^N waves per row that share the best cost found (pdp_exact_nearest_split; -1: a
plain first stage, then the rows left unproved once more at a depth chosen from their number, starting below the cost they hold): the
budget applies per cube, "nearest_work" is summed over the cubes, and "nearest_split_depth" appears on the rows searched at a depth above 0;
``--complete-nearest-rounds N`` (with ``--complete-nearest``, not with ``--complete-nearest-split``) runs that branch and bound in rounds of
2^N reads per cube (pdp_exact_nearest_round; -1: the default), cuts the open part of every tree again between two rounds and hands every
cube the best cost its row has met, from the complete search's model as the start model: the same "nearest" where it is proved,
``--complete-budget`` as the total per row, "nearest_work" summed over rounds and cubes, and "nearest_rounds" after "nearest_work".
``-c/--cpu_mode`` is rejected: the hot path has no CPU fallback.  Launched through ``python -m torch.distributed.run --nproc-per-node N``
it runs one process per GPU on a shard of the input each and reduces the result once over RCCL.
"""

import argparse
import logging
import os
import sys
from datetime import datetime

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import dimacs2json  # noqa: E402
from pdp import native  # noqa: E402
from pdp.trainer import SatFactorGraphTrainer  # noqa: E402


def _open_output(path):
    "where the result rows go: stdout, a file, or nowhere (ranks other than 0 of a sharded run: rank 0 writes the gathered rows)"
    if int(os.environ.get('RANK', '0')) != 0:
        return open(os.devnull, 'w'), True
    if not path:
        return sys.stdout, False
    return open(path, 'w'), True


def run(config, logger, output):
    "Seeds the two random sources, builds the model of config['model_type'] and writes one result row per input instance."
    complete = bool(config.get('complete'))
    if complete and config.get('split_forward'):
        raise native.NativeError("--complete does not run together with --split-forward: the exact search needs whole segments on one rank")
    if complete and config.get('isolated') and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise native.NativeError("--complete does not run together with --isolated on several ranks: the exact search needs whole segments on one rank")
    seed = config['random_seed']
    np.random.seed(seed)
    torch.manual_seed(seed)
    say = logger.info if config['verbose'] else (lambda *a, **k: None)
    say("Building the computational graph...")
    solver = SatFactorGraphTrainer(config=config, use_cuda=not config['cpu_mode'], logger=logger)
    solver._counter = 0
    solver._complete_stats = [0, 0, 0]                  # satisfiable, unsatisfiable, undecided (this rank's units)
    solver._min_unsat_stats = [0, 0]                    # optima proved, rows asked (this rank's units)
    solver._count_stats = [0, 0]                        # counts completed, rows asked (this rank's units)
    solver._sample_stats = [0, 0]                       # rows sampled, rows asked (this rank's units)
    solver._mass_stats = [0, 0]                         # solution masses proved, rows asked (this rank's units)
    solver._nearest_stats = [0, 0]                      # nearest models proved, rows asked (this rank's units)
    say("Starting the prediction phase...")
    sink, owned = _open_output(output)
    try:
        solver.predict(test_list=config['test_path'], out_file=sink, import_path_base=config['model_path'],
                       post_processor=solver._post_process_complete if complete else solver._post_process_predictions,
                       batch_replication=config['batch_replication'])
    finally:
        if owned:
            sink.close()
    if complete:
        proved = "; minimum unsatisfied clauses proved for %d of %d" % tuple(solver._min_unsat_stats) if config.get('complete_min_unsat') else ""
        counted = "; models counted for %d of %d" % tuple(solver._count_stats) if config.get('complete_count') else ""
        sampled = "; sampled %d of %d" % tuple(solver._sample_stats) if config.get('complete_sample') else ""
        massed = "; solution mass for %d of %d" % tuple(solver._mass_stats) if config.get('complete_mass') else ""
        neared = "; nearest model proved for %d of %d" % tuple(solver._nearest_stats) if config.get('complete_nearest') else ""
        say("complete search: satisfiable %d, unsatisfiable %d, undecided %d%s%s%s%s%s"
            % (tuple(solver._complete_stats) + (proved, counted, sampled, massed, neared)))
    return solver


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('model_config', help='The model configuration yaml file')
    parser.add_argument('test_path', help='The input test path')
    parser.add_argument('test_recurrence_num', help='The number of iterations for the PDP', type=int)
    parser.add_argument('-b', '--batch_replication', help='Batch replication factor', type=int, default=1)
    parser.add_argument('-z', '--batch_size', help='Batch size', type=int, default=5000)
    parser.add_argument('-m', '--max_cache_size', help='Maximum cache size', type=int, default=100000)
    parser.add_argument('-l', '--test_batch_limit', help='Memory limit for mini-batches', type=int, default=40000000)
    parser.add_argument('-w', '--local_search_iteration', help='Number of iterations for post-processing local search', type=int, default=100)
    parser.add_argument('-e', '--epsilon', help='Epsilon probablity for post-processing local search', type=float, default=0.5)
    parser.add_argument('-v', '--verbose', help='Verbose', action='store_true')
    parser.add_argument('-c', '--cpu_mode', help='Run on CPU (not available in the MI355X build)', action='store_true')
    parser.add_argument('-d', '--dimacs', help='The input folder contains DIMACS files', action='store_true')
    parser.add_argument('-s', '--random_seed', help='Random seed', type=int, default=int(datetime.now().microsecond))
    parser.add_argument('-o', '--output', help='The JSON output file', default='')
    parser.add_argument('--rng', help='Random source for random fill / Walk-SAT', choices=['torch', 'philox'], default='torch')
    parser.add_argument('--stepwise', help='Disable the persistent one-launch PDP loop', action='store_true')
    parser.add_argument('--isolated', help='Solve every instance on its own: none of the batch-wide couplings of the reference '
                        '(global minima, NaN poisoning of the whole batch); p-d-p only, results differ from the reference where those couplings act.  On several ranks (torch.distributed.run) '
                        'the instances of every forward are then spread over all GPUs',
                        action='store_true')
    parser.add_argument('--complete', help='Decide every instance with the batched exact search, the model\'s assignment as its phase hints: rows gain '
                        '"complete" (1 satisfiable, 0 unsatisfiable, -1 undecided), "pdp_solved" and "work"; not with --split-forward, nor with --isolated on several ranks',
                        action='store_true')
    parser.add_argument('--complete-budget', dest='complete_budget', help='Clause-literal reads per instance of the --complete search (0 = the library default, 2^32)',
                        type=int, default=0)
    parser.add_argument('--complete-learn', dest='complete_learn', help='With --complete: the exact search learns a clause from every conflict and backjumps '
                        '(pdp_exact_solve_learn); the same rows, far fewer reads on structured instances', action='store_true')
    parser.add_argument('--complete-certify', dest='complete_certify', help='With --complete: the learning search logs its learned clauses as a proof and '
                        'every answer is checked on the GPU (pdp_exact_check); implies --complete-learn; rows gain "certified" (1 checked, -1 undecided)',
                        action='store_true')
    parser.add_argument('--complete-core', dest='complete_core', help='With --complete --complete-certify: an "unsatisfiable" is certified by the backward '
                        'check of its proof (pdp_exact_trim) and its row gains "core": the 0-based indices, in the instance\'s clause order, of an '
                        'unsatisfiable subset of its clauses', action='store_true')
    parser.add_argument('--complete-backbone', dest='complete_backbone', help='With --complete: a satisfiable row gains "backbone", the signed 1-based '
                        'literals that hold in every model of the instance, ascending by variable (pdp_exact_solve_learn_assume, one query per '
                        'variable); literals whose query ran out of --complete-budget are left out and counted in "backbone_unknown"',
                        action='store_true')
    parser.add_argument('--complete-min-unsat', dest='complete_min_unsat', help='With --complete: every row that is not satisfiable gains "min_unsat", the '
                        'fewest clauses any assignment leaves unsatisfied (pdp_exact_min_unsat, branch and bound from the model\'s assignment, '
                        '--complete-budget reads), "min_unsat_proved" (0: the budget ran out, an upper bound), "min_unsat_solution" and "min_unsat_work"',
                        action='store_true')
    parser.add_argument('--complete-count', dest='complete_count', help='With --complete: every satisfiable row gains "model_count", the exact number of '
                        'its models (pdp_exact_count, --complete-budget reads), "model_count_log2", "model_count_proved" (0: the budget ran out, a lower '
                        'bound), "marginals" (the share of the models in which each variable is true), "marginal_gap" (the mean distance of the '
                        'soft prediction from them) and "count_work"', action='store_true')
    parser.add_argument('--complete-split', dest='complete_split', help='With --complete: spread the exact search of every instance over 2^N waves '
                        '(pdp_exact_solve_split), N from 0 to 16, or -1: a plain first stage, then the undecided instances at a depth that fills the GPU; '
                        'the same "complete" and solution, "work" summed over the cubes, "split_depth" on the rows searched at a depth above 0; '
                        'not with --complete-learn or --complete-certify', type=int, default=None)
    parser.add_argument('--complete-rounds', dest='complete_rounds', help='With --complete: run the exact search in rounds of 2^N reads per cube '
                        '(pdp_exact_solve_round), N from 0 to 40, or -1 for the default; between two rounds the open part of every search tree is '
                        'cut again to fill the GPU, and --complete-budget is the total of reads per row over all rounds and cubes; the same '
                        '"complete", a model of the instance as the solution (not always the plain search\'s), "work" summed over the rounds and '
                        'cubes, "complete_rounds" on every row searched this way; not with --complete-split, --complete-learn or '
                        '--complete-certify', type=int, default=None)
    parser.add_argument('--complete-count-split', dest='complete_count_split', help='With --complete --complete-count: spread the count of every '
                        'satisfiable row over 2^N waves (pdp_exact_count_split), N from 0 to 16, or -1: a plain first count, then the rows that ran '
                        'out of its reads once more at a depth that fills the GPU; the same counts and marginals, "count_work" summed over the cubes, '
                        '"count_split_depth" on the rows counted at a depth above 0', type=int, default=None)
    parser.add_argument('--complete-count-rounds', dest='complete_count_rounds', help='With --complete --complete-count: count in rounds of 2^N '
                        'reads per cube (pdp_exact_count_round), N from 0 to 40, or -1 for the default; between two rounds the open part of '
                        'every search tree is cut again to fill the GPU, and --complete-budget is the total of reads per row over all rounds; the '
                        'same counts and marginals, "count_work" summed over the rounds and cubes, "count_rounds" on every counted row; not '
                        'with --complete-count-split', type=int, default=None)
    parser.add_argument('--complete-min-unsat-split', dest='complete_min_unsat_split', help='With --complete --complete-min-unsat: spread the branch '
                        'and bound of every row over 2^N waves that share the best cost found (pdp_exact_min_unsat_split), N from 0 to 16, or -1: a '
                        'plain first stage, then the rows whose optimum is not proved once more, from the cost reached, at a depth that fills the '
                        'GPU; "min_unsat" and "min_unsat_proved" mean the same, "min_unsat_work" is summed over the cubes, '
                        '"min_unsat_split_depth" on the rows searched at a depth above 0', type=int, default=None)
    parser.add_argument('--complete-sample', dest='complete_sample', help='With --complete --complete-count: every row whose count is proved and '
                        'exact (at most 2^53) gains "samples", K models in the format of "solution" drawn uniformly, with replacement, from all its '
                        'models (pdp_exact_models_at at uniform ranks below the count; the seed is -s), and "sample_ranks", the ranks drawn',
                        type=int, default=None, metavar='K')
    parser.add_argument('--complete-mass', dest='complete_mass', help='With --complete: every satisfiable row gains "solution_mass", the probability '
                        'that rounding every variable independently with the soft prediction gives a model (pdp_exact_mass, --complete-budget '
                        'reads), "solution_mass_log2", "solution_mass_open" (the mass not visited: the true value lies in [solution_mass, '
                        'solution_mass + solution_mass_open]), "solution_mass_proved" (0: the budget ran out), "posterior" (per variable, '
                        'P(true | the draw is a model)) and "mass_work"; after Walk-SAT (-w above 0) the prediction is 0/1 and the mass 1 or 0: '
                        'meant for -w 0', action='store_true')
    parser.add_argument('--complete-mass-split', dest='complete_mass_split', help='With --complete --complete-mass: spread the weighted search of '
                        'every satisfiable row over 2^N waves (pdp_exact_mass_split), N from 0 to 16, or -1: a plain first stage, then the rows '
                        'that ran out of its reads once more at a depth that fills the GPU; the budget applies per cube, "mass_work" is summed '
                        'over the cubes, "mass_split_depth" on the rows weighed at a depth above 0', type=int, default=None)
    parser.add_argument('--complete-nearest', dest='complete_nearest', help='With --complete: every satisfiable row gains "nearest", the fewest '
                        'variables in which a model of the instance differs from the model\'s assignment (pdp_exact_nearest, branch and bound from '
                        'that assignment, --complete-budget reads; left out where no model was met), "nearest_proved" (0: the budget ran out, an '
                        'upper bound), "nearest_solution" and "nearest_work"; a row PDP solved gets "nearest" 0', action='store_true')
    parser.add_argument('--complete-nearest-split', dest='complete_nearest_split', help='With --complete --complete-nearest: spread the branch '
                        'and bound of every satisfiable row over 2^N waves that share the best cost found (pdp_exact_nearest_split), N from 0 to '
                        '16, or -1: a plain first stage, then the rows left unproved once more at a depth that fills the GPU, starting below the '
                        'cost of the model they hold; the budget applies per cube, "nearest_work" is summed over the cubes, '
                        '"nearest_split_depth" on the rows searched at a depth above 0.  The model --complete found is always the start model of '
                        'that search, so N = 0 is not the call without the flag: the start model is checked first and its reads are part of '
                        '"nearest_work"', type=int, default=None)
    parser.add_argument('--complete-nearest-rounds', dest='complete_nearest_rounds', help='With --complete --complete-nearest: run the branch '
                        'and bound of every satisfiable row in rounds of 2^N reads per cube (pdp_exact_nearest_round), N from 0 to 40, or -1 for '
                        'the default; between two rounds the open part of every search tree is cut again to fill the GPU and every cube is '
                        'handed the best cost its row has met, and --complete-budget is the total of reads per row over all rounds and cubes; '
                        'the model --complete found is the start model; the same "nearest" where it is proved, "nearest_work" summed over the '
                        'rounds and cubes, "nearest_rounds" after "nearest_work"; not with --complete-nearest-split', type=int, default=None)
    parser.add_argument('--split-forward', dest='split_forward', help='On several ranks: spread EVERY forward over all GPUs (one contiguous instance range '
                        'per rank) and keep the couplings of the reference -- its batch-wide reductions are completed across the ranks chunk by chunk; '
                        'p-d-p, -b 1; the rows are those of the single-process run', action='store_true')
    args = vars(parser.parse_args(argv))
    if args['complete_learn'] and not args['complete']:
        parser.error("--complete-learn selects the search of --complete: give --complete as well")
    if args['complete_certify'] and not args['complete']:
        parser.error("--complete-certify checks the answers of --complete: give --complete as well")
    if args['complete_core'] and not args['complete_certify']:
        parser.error("--complete-core names the core of a certified answer: give --complete-certify as well")
    if args['complete_backbone'] and not args['complete']:
        parser.error("--complete-backbone names the backbone of an answer of --complete: give --complete as well")
    if args['complete_min_unsat'] and not args['complete']:
        parser.error("--complete-min-unsat bounds the rows --complete leaves unsatisfied: give --complete as well")
    if args['complete_count'] and not args['complete']:
        parser.error("--complete-count counts the models of the rows --complete satisfies: give --complete as well")
    if args['complete_mass'] and not args['complete']:
        parser.error("--complete-mass weighs the models of the rows --complete satisfies: give --complete as well")
    if args['complete_nearest'] and not args['complete']:
        parser.error("--complete-nearest measures the rows --complete satisfies: give --complete as well")
    if args['complete_split'] is not None:
        if not args['complete']:
            parser.error("--complete-split spreads the search of --complete: give --complete as well")
        if args['complete_learn'] or args['complete_certify']:
            parser.error("--complete-split spreads the plain search: give it without --complete-learn and --complete-certify")
        if not -1 <= args['complete_split'] <= 16:
            parser.error("--complete-split takes a depth from 0 to 16, or -1 for a depth chosen from the undecided instances")
    if args['complete_rounds'] is not None:
        if not args['complete']:
            parser.error("--complete-rounds runs the search of --complete in rounds: give --complete as well")
        if args['complete_split'] is not None:
            parser.error("--complete-rounds cuts the search between its rounds: give it without --complete-split")
        if args['complete_learn'] or args['complete_certify']:
            parser.error("--complete-rounds runs the plain search: give it without --complete-learn and --complete-certify")
        if not -1 <= args['complete_rounds'] <= 40:
            parser.error("--complete-rounds takes log2 of the reads per cube and round, from 0 to 40, or -1 for the default")
    if args['complete_count_split'] is not None:
        if not args['complete_count']:
            parser.error("--complete-count-split spreads the count of --complete-count: give --complete-count as well")
        if not -1 <= args['complete_count_split'] <= 16:
            parser.error("--complete-count-split takes a depth from 0 to 16, or -1 for a depth chosen from the rows that ran out")
    if args['complete_count_rounds'] is not None:
        if not args['complete_count']:
            parser.error("--complete-count-rounds counts the models of --complete-count in rounds: give --complete-count as well")
        if args['complete_count_split'] is not None:
            parser.error("--complete-count-rounds cuts the search between its rounds: give it without --complete-count-split")
        if not -1 <= args['complete_count_rounds'] <= 40:
            parser.error("--complete-count-rounds takes log2 of the reads per cube and round, from 0 to 40, or -1 for the default")
    if args['complete_mass_split'] is not None:
        if not args['complete_mass']:
            parser.error("--complete-mass-split spreads the search of --complete-mass: give --complete-mass as well")
        if not -1 <= args['complete_mass_split'] <= 16:
            parser.error("--complete-mass-split takes a depth from 0 to 16, or -1 for a depth chosen from the rows that ran out")
    if args['complete_min_unsat_split'] is not None:
        if not args['complete_min_unsat']:
            parser.error("--complete-min-unsat-split spreads the search of --complete-min-unsat: give --complete-min-unsat as well")
        if not -1 <= args['complete_min_unsat_split'] <= 16:
            parser.error("--complete-min-unsat-split takes a depth from 0 to 16, or -1 for a depth chosen from the rows left unproved")
    if args['complete_nearest_split'] is not None:
        if not args['complete_nearest']:
            parser.error("--complete-nearest-split spreads the search of --complete-nearest: give --complete-nearest as well")
        if not -1 <= args['complete_nearest_split'] <= 16:
            parser.error("--complete-nearest-split takes a depth from 0 to 16, or -1 for a depth chosen from the rows left unproved")
    if args['complete_nearest_rounds'] is not None:
        if not args['complete_nearest']:
            parser.error("--complete-nearest-rounds runs the search of --complete-nearest in rounds: give --complete-nearest as well")
        if args['complete_nearest_split'] is not None:
            parser.error("--complete-nearest-rounds cuts the search between its rounds: give it without --complete-nearest-split")
        if not -1 <= args['complete_nearest_rounds'] <= 40:
            parser.error("--complete-nearest-rounds takes log2 of the reads per cube and round, from 0 to 40, or -1 for the default")
    if args['complete_sample'] is not None:
        if not args['complete_count']:
            parser.error("--complete-sample draws from the models --complete-count counts: give --complete-count as well")
        if args['complete_sample'] < 1:
            parser.error("--complete-sample takes the number of models to draw per row, at least 1")
    if args['complete_certify']:
        args['complete_learn'] = True

    with open(args['model_config'], 'r') as f:
        model_config = yaml.safe_load(f)

    fmt = '[%(levelname)s] %(asctime)s - %(name)s: %(message)s'
    logging.basicConfig(level=logging.DEBUG, format=fmt)
    logger = logging.getLogger(model_config['model_name'])

    # -d: the reference converts the DIMACS input into a temporary JSON file first (satyr.py:66-80); here the loader reads the
    # DIMACS files directly through the native parser (same instances, same order, same labels -- dataset.dimacs_file_list)
    temp_file_name = None
    if args['dimacs'] and args['verbose']:
        logger.info("Reading DIMACS files...")

    config = {**model_config, **args}
    if config['model_type'] in ('p-d-p', 'walk-sat', 'reinforce'):
        config['model_path'] = None
        config['hidden_dim'] = 3
    if config['model_type'] == 'walk-sat':
        config['local_search_iteration'] = config['test_recurrence_num']
    config['dropout'] = 0
    config['error_dim'] = 1
    config['exploration'] = 0
    config['persistent'] = not config['stepwise']

    # one process per GPU under torch.distributed.run: instances are sharded across the ranks (pdp/factorgraph/base.py::predict)
    # PDP_DIST_FORCE=1 joins the process group at world size 1 as well (torch.distributed.run --nproc-per-node 1): the all-reduce and the
    # row gather then run through RCCL on a one-GPU box exactly as they do on eight
    world = int(os.environ.get('WORLD_SIZE', '1'))
    grouped = world > 1 or (os.environ.get('PDP_DIST_FORCE') == '1' and 'RANK' in os.environ)
    if grouped:
        import torch.distributed as dist
        # PDP_DIST_BACKEND=gloo lets several ranks share one GPU (checks of the sharded path on a single-GPU box); RCCL needs one GPU each
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % max(1, torch.cuda.device_count()))
        dist.init_process_group(backend=os.environ.get('PDP_DIST_BACKEND', 'nccl'))
    try:
        run(config, logger, config['output'])
    finally:
        if temp_file_name is not None and os.path.exists(temp_file_name):
            os.remove(temp_file_name)
        if grouped:
            import torch.distributed as dist
            dist.destroy_process_group()
    if world == 1 or int(os.environ.get('RANK', '0')) == 0:
        print('')


if __name__ == '__main__':
    main()
