"""Model factory + prediction post-processing for PDP SAT solvers (reference: src/pdp/trainer.py).

The inference side of ``SatFactorGraphTrainer``: ``_build_graph`` (model_type -> solver class,
trainer.py:48-99), ``_check_recurrence_termination`` (:150-162), ``_post_process_predictions`` (:125-148; ``_post_process_complete``: the same rows
decided by the hinted exact search, satyr.py --complete; with --complete-count the satisfiable rows' models counted, and with
--complete-count-split that count spread over 2^depth waves per row, pdp_exact_count_split, with --complete-sample K uniform samples of
those models, pdp_exact_models_at) and the test-mode
metrics ``_compute_evaluation_metrics`` (:108-123: accuracy / recall errors of the clause check and the energy loss), and the training
loss ``_compute_loss`` (:100-106) used by ``FactorGraphTrainerBase._train_batch``.
"""

import numpy as np
import torch
import torch.nn as nn

from pdp import native
from pdp.factorgraph.base import FactorGraphTrainerBase
from pdp.nn import solver, util


class Perceptron(nn.Module):
    "1-hidden-layer perceptron with sigmoid output (reference: trainer.py:20-29); classifier head of the neural predictor."

    def __init__(self, input_dimension, hidden_dimension, output_dimension):
        super(Perceptron, self).__init__()
        self._layer1 = nn.Linear(input_dimension, hidden_dimension)
        self._layer2 = nn.Linear(hidden_dimension, output_dimension, bias=False)

    def forward(self, inp):
        return torch.sigmoid(self._layer2(torch.relu(self._layer1(inp))))


class SatFactorGraphTrainer(FactorGraphTrainerBase):
    "Builds a PDP SAT solver from a config dict and runs prediction (reference: trainer.py:34-162)."

    def __init__(self, config, use_cuda, logger):
        super(SatFactorGraphTrainer, self).__init__(config=config, has_meta_data=False, error_dim=config.get('error_dim', 3),
                                                    loss=None, evaluator=nn.L1Loss(), use_cuda=use_cuda, logger=logger)
        self._eps = 1e-8 * torch.ones(1, device=self._device)
        self._loss_evaluator = util.SatLossEvaluator(alpha=self._config.get('exploration', 0.0), device=self._device)
        self._cnf_evaluator = util.SatCNFEvaluator(device=self._device)
        self._counter = 0
        self._max_coeff = 10.0

    def _build_graph(self, config):
        rng = config.get('rng', 'torch')
        seed = int(config.get('random_seed', 0) or 0)
        t = config['model_type']
        common = dict(local_search_iterations=config['local_search_iteration'], epsilon=config['epsilon'], rng=rng, seed=seed)
        if t == 'p-d-p':
            model = solver.SurveyPropagatorSolver(device=self._device, name=config['model_name'], tolerance=config['tolerance'],
                                                  t_max=config['t_max'], persistent=config.get('persistent', True), **common)
            model._isolated = bool(config.get('isolated', False))
        elif t == 'walk-sat':
            model = solver.WalkSATSolver(device=self._device, name=config['model_name'],
                                         iteration_num=config['local_search_iteration'], epsilon=config['epsilon'], rng=rng, seed=seed)
        elif t == 'reinforce':
            model = solver.ReinforceSurveyPropagatorSolver(device=self._device, name=config['model_name'], pi=config['pi'],
                                                           decimation_probability=config['decimation_probability'],
                                                           persistent=config.get('persistent', True), **common)
        elif t in ('np-nd-np', 'np-d-np', 'p-nd-np'):
            model = solver.build_neural_solver(self._device, config, Perceptron, common)
            if hasattr(model._propagator, '_drop_out'):
                # where the training path's dropout masks come from: the device generator (default), or -- dropout_rng: 'torch' -- the global
                # CPU stream drawn exactly as the reference's --cpu_mode run draws it (the golden tests; it builds every mask on the host)
                model._propagator._rng = config.get('dropout_rng', 'device')
            # random initial states (training / test mode): the reference's CPU stream by default, 'device' for throughput
            for plug_in in (model._propagator, model._decimator):
                plug_in._init_rng = config.get('init_rng', 'torch')
            if config.get('dropout', 0) or config.get('init_rng', 'torch') != 'torch':
                # said once: a YAML with `rng: torch` and a seed no longer pins these two streams to the reference's --cpu_mode draws by itself
                self._logger.info("random sources: dropout masks from %r (config key dropout_rng), random initial states from %r (init_rng), random fill / "
                                  "Walk-SAT from %r (rng); 'torch' = the reference's global CPU stream" % (model._propagator._rng if hasattr(model._propagator, '_rng') else 'n/a',
                                                                                                        config.get('init_rng', 'torch'), rng))
        else:
            raise KeyError("unknown model_type %r" % (t,))
        if config.get('verbose'):
            self._logger.info("The model parameter count is %d." % model.parameter_count())
        return [model]

    def _compute_loss(self, model, loss, prediction, label, graph_map, batch_variable_map, batch_function_map, edge_feature, meta_data):
        "the energy of the prediction (reference: trainer.py:100-106); differentiable with respect to the prediction"
        return self._loss_evaluator(variable_prediction=prediction[0], label=label, graph_map=graph_map, batch_variable_map=batch_variable_map,
                                    batch_function_map=batch_function_map, edge_feature=edge_feature, meta_data=meta_data,
                                    global_step=model._global_step, eps=self._eps, max_coeff=self._max_coeff,
                                    loss_sharpness=self._config['loss_sharpness'], sat_problem=getattr(model, '_last_problem', None))

    def _compute_evaluation_metrics(self, model, evaluator, prediction, label, graph_map, batch_variable_map, batch_function_map,
                                    edge_feature, meta_data):
        """[accuracy error, recall error, energy loss] of a prediction on a labelled batch (reference: trainer.py:108-123).
        The clause check and the loss run on the problem the model has just solved (no mask rebuild)."""
        sat_problem = getattr(model, '_last_problem', None)
        output, _ = self._cnf_evaluator(variable_prediction=prediction[0], graph_map=graph_map, batch_variable_map=batch_variable_map,
                                        batch_function_map=batch_function_map, edge_feature=edge_feature, meta_data=meta_data,
                                        sat_problem=sat_problem)
        output = (output.reshape(label.shape) > 0.5).float()
        recall = torch.sum(label * (output - label).abs()) / torch.max(torch.sum(label), self._eps)
        accuracy = evaluator(output, label).unsqueeze(0)
        loss_value = self._loss_evaluator(variable_prediction=prediction[0], label=label, graph_map=graph_map,
                                          batch_variable_map=batch_variable_map, batch_function_map=batch_function_map,
                                          edge_feature=edge_feature, meta_data=meta_data, global_step=model._global_step,
                                          eps=self._eps, max_coeff=self._max_coeff, loss_sharpness=self._config['loss_sharpness'],
                                          sat_problem=sat_problem).unsqueeze(0)
        return torch.cat([accuracy, recall.reshape(1), loss_value], 0)

    def _prediction_rows(self, model, prediction, graph_map, batch_variable_map, batch_function_map, edge_feature, graph_feat, label, misc_data):
        "the result rows of a forward as dictionaries (the reference's five keys in its order) and the variable offsets of the instances"
        sat_problem = getattr(model, '_last_problem', None)
        solved, unsat = self._cnf_evaluator(prediction[0], graph_map, batch_variable_map, batch_function_map, edge_feature,
                                            graph_feat, sat_problem=sat_problem)
        output = solved.detach().cpu().numpy()
        unsat_clause_num = unsat.detach().cpu().numpy()
        labs = label.detach().cpu().numpy()
        bits = (prediction[0].detach().reshape(-1) > 0.5).to(torch.uint8).cpu().numpy()
        counts = np.bincount(batch_variable_map.detach().cpu().numpy().astype(np.int64), minlength=output.shape[0])
        offs = np.concatenate(([0], np.cumsum(counts)))
        rows = []
        for i in range(output.shape[0]):
            rows.append({
                'ID': misc_data[i][0] if len(misc_data[i]) > 0 else "",
                'label': int(labs[i, 0]),
                'solved': int(output[i].flatten()[0] == 1),
                'unsat_clauses': int(unsat_clause_num[i].flatten()[0]),
                'solution': bits[offs[i]:offs[i + 1]].astype(int).tolist()
            })
        return rows, offs

    def _write_rows(self, rows):
        "the rows as text, counted as written"
        self._counter += len(rows)
        if hasattr(self, '_run_stats'):
            self._run_stats[0] += len(rows); self._run_stats[1] += sum(r['solved'] for r in rows)
            self._run_stats[2] += sum(r['unsat_clauses'] for r in rows)
        # a None (solution_mass_log2 at mass 0; model_count_log2 would hold one at a count of 0) is written as JSON's null
        return "".join(str(r).replace("'", '"').replace(': None', ': null') + "\n" for r in rows)

    def _post_process_predictions(self, model, prediction, graph_map, batch_variable_map, batch_function_map,
                                  edge_feature, graph_feat, label, misc_data):
        """JSON result rows (reference: trainer.py:125-148).  The reference scans ``batch_variable_map == i`` for every
        instance (O(B*V)); instance slices come from one prefix sum here."""
        rows, _ = self._prediction_rows(model, prediction, graph_map, batch_variable_map, batch_function_map, edge_feature, graph_feat, label,
                                        misc_data)
        return self._write_rows(rows)

    def _post_process_complete(self, model, prediction, graph_map, batch_variable_map, batch_function_map,
                               edge_feature, graph_feat, label, misc_data):
        """The rows of ``_post_process_predictions`` completed by the exact search (satyr.py --complete): the prediction is the phase hint of
        pdp_exact_solve_hinted on the unreplicated instances of the forward.  Every row gains "complete" (1 satisfiable, 0 unsatisfiable, -1
        undecided within config['complete_budget'] clause-literal reads), "pdp_solved" (what "solved" is without the search) and "work" (the
        reads of the search); with config['complete_certify'] also "certified" (1: the answer passed pdp_exact_check, -1: undecided), and with config['complete_core'] an
        unsatisfiable row also "core", the 0-based indices (in the instance's clause order) of the clauses its refutation rests on.  A satisfiable row gets solved 1, unsat_clauses 0 and the search's model -- PDP's own assignment where PDP had
        solved the instance, because the check pass accepts it; every other row keeps its five reference keys.  With config['complete_backbone']
        a satisfiable row also gains "backbone", the signed 1-based literals that hold in every model (ascending by variable; one query of
        the search under assumptions per variable, all instances of the forward in one batch), and, when queries ran out of budget,
        "backbone_unknown" with their count (those literals are left out).  With config['complete_min_unsat'] every row whose "complete" is not 1
        also gains "min_unsat" (the fewest unsatisfied clauses pdp_exact_min_unsat found from PDP's assignment, within the same budget),
        "min_unsat_proved" (1: that is the minimum over all assignments, 0: an upper bound), "min_unsat_solution" and "min_unsat_work";
        its five reference keys stay PDP's.  With config['complete_min_unsat_split'] (a depth 0..16, or -1: exact.min_unsat_split's 'auto') that
        search runs with every row spread over 2^depth waves that share the best cost found (pdp_exact_min_unsat_split): "min_unsat" and
        "min_unsat_proved" mean the same, which minimiser "min_unsat_solution" is and "min_unsat_work" depend on the timing of the cubes, and a
        row searched at a depth above 0 gains "min_unsat_split_depth" after "min_unsat_work".  With config['complete_split'] (a depth 0..16, or -1: exact.split_solve's 'auto') the same search runs
        with every instance spread over 2^depth waves (pdp_exact_solve_split): "complete" and the solution are unchanged, "work" is the sum over
        the cubes, and a row searched at a depth above 0 gains "split_depth" after "work".  With config['complete_rounds'] (log2 of the reads per cube
        and round, or -1: the default) the search runs in rounds instead (exact.solve_rounds, pdp_exact_solve_round; no check pass, so the
        solution of a row PDP had solved is a model the hints lead to, not always PDP's own): the budget is the total per row over all
        rounds and cubes, and every row that had a cube gains "complete_rounds" after "work".  With config['complete_count'] every row whose "complete" is 1 gains "model_count" (pdp_exact_count within
        the same budget: an int while it is exact, a float above 2^53), "model_count_log2", "model_count_proved" (1: the number of models, 0: the budget
        ran out, a lower bound), "marginals" (per variable, the share of the counted models in which it is true), "marginal_gap" (the mean
        over the variables of |the soft prediction - marginal|) and "count_work"; marginals and marginal_gap are left out where nothing was
        counted, and an instance of more than 1023 variables keeps its row as it is.  With config['complete_count_split'] (a depth 0..16, or
        -1: exact.count_split's 'auto') that count runs with every instance spread over 2^depth waves (pdp_exact_count_split): the same
        counts and marginals while no budget runs out, "count_work" is the sum over the cubes, and a row counted at a depth above 0 gains
        "count_split_depth" after "count_work".  With config['complete_count_rounds'] (log2 of the reads per cube and round, or -1: the
        default) the count runs in rounds instead (exact.count_rounds, pdp_exact_count_round): the budget is the total per row over all
        rounds, and every counted row gains "count_rounds" after "count_work".  With config['complete_sample'] (K >= 1, with complete_count) every row whose count is proved and
        exact (at most 2^53, above 0) gains "samples", K models in the format of "solution" drawn uniformly with replacement from ALL its
        models (exact.sample_models: uniform ranks below the count, then pdp_exact_models_at; the seed is config['random_seed'], the stream
        that of the row's position among the forward's satisfiable rows), and "sample_ranks", the ranks drawn; every other row is unchanged.
        With config['complete_mass'] (independent of complete_count) every row whose "complete" is 1 gains "solution_mass" (pdp_exact_mass
        within the same budget, the weights being the row's slice of the soft prediction that also serves as hints: the probability that
        rounding every variable independently with it gives a model), "solution_mass_log2" (None at 0), "solution_mass_open" (the mass
        of the part of the tree not visited: the true value lies in [solution_mass, solution_mass + solution_mass_open]),
        "solution_mass_proved" (1 / 0), "posterior" (per variable, P(true | the draw is a model); left out where the mass is 0) and
        "mass_work"; a row of more than 1023 variables or with a prediction outside [0, 1] stays as it is.  After Walk-SAT the prediction
        is 0/1, so the mass is 1 or 0 and costs one descent.  With config['complete_mass_split'] (a depth 0..16, or -1: exact.mass_split's
        'auto') that search runs with every row spread over 2^depth waves (pdp_exact_mass_split): the budget applies per cube, "mass_work" is
        the sum over the cubes, and a row weighed at a depth above 0 gains "mass_split_depth" after "mass_work".  With
        config['complete_nearest'] every row whose "complete" is 1 gains "nearest" (pdp_exact_nearest within the same budget from the
        same slice of the prediction, all penalties 1: the fewest variables in which a model differs from PDP's assignment; left out
        where no model was met within the budget), "nearest_proved" (1: that is the minimum over all models, 0: an upper bound or
        nothing), "nearest_solution" (that model, in the format of "solution") and "nearest_work"; a row PDP solved costs one check pass
        and gets "nearest" 0.  With config['complete_nearest_split'] (a depth 0..16, or -1: exact.nearest_split's 'auto') that search runs
        with every row spread over 2^depth waves that share the best cost found (pdp_exact_nearest_split), from the complete search's model
        as its start model: "nearest", "nearest_proved" and "nearest_solution" mean the same, which nearest model comes back and
        "nearest_work" (the sum over the cubes) depend on the timing of the cubes, and a row searched at a depth above 0 gains
        "nearest_split_depth" after "nearest_work".  With config['complete_nearest_rounds'] (log2 of the reads per cube and round, or -1: the
        default) it runs in rounds instead (exact.nearest_rounds, pdp_exact_nearest_round), again from the complete search's model: the
        budget is the total per row over all rounds and cubes, every output is a function of the inputs, and every row gains
        "nearest_rounds" after "nearest_work"."""
        rows, offs = self._prediction_rows(model, prediction, graph_map, batch_variable_map, batch_function_map, edge_feature, graph_feat, label,
                                           misc_data)
        sat_problem = getattr(model, '_last_problem', None)
        handle = None
        if sat_problem is not None and sat_problem._orig[0] is graph_map:
            handle = sat_problem._native if sat_problem._batch_replication == 1 else sat_problem._native_unreplicated()
        if handle is None or handle.R != 1 or handle.V != int(offs[-1]):
            handle = native.Problem(graph_map, batch_variable_map, batch_function_map, edge_feature, batch_size=len(rows))
        hint = prediction[0].detach().reshape(-1).to(torch.float32).contiguous()
        budget = int(self._config.get('complete_budget', 0) or 0)
        certified = split_depth = used_rounds = None
        if self._config.get('complete_certify'):
            # the learning search with its lemma log, every answer checked (pdp_exact_check); a proof that did not fit its region is
            # logged once more into regions of the size the first run reported; a refuted answer raises
            from pdp import exact
            names = ['%d (%s)' % (i, row['ID']) for i, row in enumerate(rows)]
            # config['complete_core']: the unsatisfiable answers are judged by the backward check (pdp_exact_trim), which also names the core
            counts = None
            if self._config.get('complete_core'):
                counts = torch.bincount(handle.export_graph()[2].long(), minlength=handle.B)[:handle.B].cpu().numpy()
            status, solution, work, certified, plen, size, _, cores = exact._certified(handle, budget, hint, 0, names, counts=counts)
            if ((status != -1) & (plen > size)).any():
                off = torch.from_numpy(np.concatenate([[0], np.cumsum(plen)]).astype(np.int64)).to(hint.device)
                status, solution, work, certified, _, _, _, cores = exact._certified(handle, budget, hint, 0, names, proof_off=off, counts=counts)
            solution = solution.astype(int)
        elif self._config.get('complete_split') is not None:
            # config['complete_split']: the same search with every instance spread over 2^depth waves (pdp_exact_solve_split); -1: auto
            from pdp import exact
            split = int(self._config['complete_split'])
            status, solution, work, split_depth = exact.split_solve(
                handle, lambda: exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows)), budget, hint,
                'auto' if split < 0 else split, hint.device)
            solution = solution.astype(int)
        elif self._config.get('complete_rounds') is not None:
            # config['complete_rounds']: the same search in rounds of 2^N reads per cube (pdp_exact_solve_round); -1: the default
            from pdp import exact
            per_round = int(self._config['complete_rounds'])
            status, solution, work, used_rounds = exact.solve_rounds(
                handle, lambda: exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows)), budget, hint,
                None if per_round < 0 else 1 << per_round, None, None, hint.device)
            solution = solution.astype(int)
        else:
            status, solution, work = handle.exact_solve(budget, hints=hint, learn=bool(self._config.get('complete_learn')))
            status, work = status.cpu().numpy(), work.cpu().numpy()
            solution = solution.cpu().numpy().astype(int)
        for i, row in enumerate(rows):
            row['complete'], row['pdp_solved'], row['work'] = int(status[i]), row['solved'], int(work[i])
            if split_depth is not None and split_depth[i] > 0:
                row['split_depth'] = int(split_depth[i])
            if used_rounds is not None and used_rounds[i] > 0:
                row['complete_rounds'] = int(used_rounds[i])
            if certified is not None:
                row['certified'] = int(certified[i])
                if cores[i] is not None:
                    row['core'] = [int(c) for c in cores[i]]
            if status[i] == 1:
                row['solved'], row['unsat_clauses'], row['solution'] = 1, 0, solution[offs[i]:offs[i + 1]].tolist()
        if self._config.get('complete_backbone'):
            from pdp import exact
            items = exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows))
            models = [np.asarray(solution[offs[i]:offs[i + 1]], dtype=np.float32) for i in range(len(rows))]
            for row, bb in zip(rows, exact.backbone_of(items, np.asarray(status), models, budget=budget, device=hint.device)):
                if bb is not None:
                    row['backbone'] = [int(v + 1) * int(bb[v]) for v in np.nonzero(np.abs(bb) == 1)[0]]
                    if (bb == 2).any():
                        row['backbone_unknown'] = int((bb == 2).sum())
        if self._config.get('complete_min_unsat'):
            # the rows the search did not satisfy, once more, as one batch of their own: the fewest unsatisfied clauses from PDP's assignment
            from pdp import exact
            open_rows = [i for i in range(len(rows)) if status[i] != 1]
            if open_rows:
                items = exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows))
                pred = hint.cpu().numpy()
                # config['complete_min_unsat_split']: every row spread over 2^depth waves (pdp_exact_min_unsat_split); -1: auto
                msplit = self._config.get('complete_min_unsat_split')
                msplit = None if msplit is None else ('auto' if int(msplit) < 0 else int(msplit))
                st, cost, models, mwork, mdepth = exact.min_unsat([items[i] for i in open_rows], budget=budget, device=hint.device,
                                                                  hints=[pred[offs[i]:offs[i + 1]] for i in open_rows], split=msplit, depths=True)
                for k, i in enumerate(open_rows):
                    rows[i]['min_unsat'], rows[i]['min_unsat_proved'] = int(cost[k]), int(st[k] == 1)
                    rows[i]['min_unsat_solution'], rows[i]['min_unsat_work'] = models[k].astype(int).tolist(), int(mwork[k])
                    if mdepth[k] > 0:
                        rows[i]['min_unsat_split_depth'] = int(mdepth[k])
                if hasattr(self, '_min_unsat_stats'):
                    self._min_unsat_stats[0] += int((st == 1).sum()); self._min_unsat_stats[1] += len(open_rows)
        if self._config.get('complete_count'):
            # the satisfiable rows, once more, as one batch of their own: how many models, and how far every variable is from being forced
            from pdp import exact
            sat_rows = [i for i in range(len(rows)) if status[i] == 1]
            if sat_rows:
                items = exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows))
                pred = hint.cpu().numpy().astype(np.float64)
                # config['complete_count_split']: the count of every row spread over 2^depth waves (pdp_exact_count_split); -1: auto
                csplit = self._config.get('complete_count_split')
                csplit = None if csplit is None else ('auto' if int(csplit) < 0 else int(csplit))
                # config['complete_count_rounds']: the count in rounds of 2^N reads per cube (pdp_exact_count_round); -1: the default
                crounds = self._config.get('complete_count_rounds')
                if crounds is not None:
                    st, count, marginals, cwork, cdepth = exact.count_models(
                        [items[i] for i in sat_rows], budget=budget, device=hint.device, split='rounds',
                        round_budget=None if int(crounds) < 0 else 1 << int(crounds), depths=True)
                    cdepth, crounds = np.zeros(len(sat_rows), dtype=np.int8), cdepth
                else:
                    st, count, marginals, cwork, cdepth = exact.count_models([items[i] for i in sat_rows], budget=budget, device=hint.device,
                                                                             split=csplit, depths=True)
                exact_int = exact.count_is_exact(st, count)
                for k, i in enumerate(sat_rows):
                    if st[k] == -2:
                        continue                                        # more than 1023 variables: not counted, the row stays as it is
                    row = rows[i]
                    row['model_count'] = int(count[k]) if exact_int[k] else float(count[k])
                    row['model_count_log2'] = float(np.log2(count[k])) if count[k] > 0 else None
                    row['model_count_proved'] = int(st[k] == 1)
                    if count[k] > 0:
                        row['marginals'] = marginals[k].tolist()
                        row['marginal_gap'] = float(np.mean(np.abs(pred[offs[i]:offs[i + 1]] - marginals[k])))
                    row['count_work'] = int(cwork[k])
                    if cdepth[k] > 0:
                        row['count_split_depth'] = int(cdepth[k])
                    if crounds is not None:
                        row['count_rounds'] = int(crounds[k])
                if hasattr(self, '_count_stats'):
                    self._count_stats[0] += int((st == 1).sum()); self._count_stats[1] += len(sat_rows)
                if self._config.get('complete_sample'):
                    # config['complete_sample']: K models of every row with an exact count, drawn uniformly from all of them (exact.sample_models)
                    samples, sranks = exact.sample_models([items[i] for i in sat_rows], int(self._config['complete_sample']),
                                                          seed=int(self._config.get('random_seed', 0) or 0), budget=budget, counts=(st, count),
                                                          device=hint.device)
                    for k, i in enumerate(sat_rows):
                        if samples[k] is not None:
                            rows[i]['samples'] = samples[k].astype(int).tolist()
                            rows[i]['sample_ranks'] = [int(r) for r in sranks[k]]
                    if hasattr(self, '_sample_stats'):
                        self._sample_stats[0] += sum(s is not None for s in samples); self._sample_stats[1] += len(sat_rows)
        if self._config.get('complete_mass'):
            # the satisfiable rows, once more, as one batch of their own: how much of the soft prediction's own mass lies on models
            from pdp import exact
            sat_rows = [i for i in range(len(rows)) if status[i] == 1]
            if sat_rows:
                items = exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows))
                pred = hint.cpu().numpy()
                # config['complete_mass_split']: the search of every row spread over 2^depth waves (pdp_exact_mass_split); -1: auto
                zsplit = self._config.get('complete_mass_split')
                zsplit = None if zsplit is None else ('auto' if int(zsplit) < 0 else int(zsplit))
                st, mass, posterior, open_mass, zwork, zdepth = exact.solution_mass([items[i] for i in sat_rows],
                                                                                    [pred[offs[i]:offs[i + 1]] for i in sat_rows], budget=budget,
                                                                                    device=hint.device, split=zsplit, depths=True)
                for k, i in enumerate(sat_rows):
                    if st[k] in (-2, -3):
                        continue                # more than 1023 variables, or a prediction that is not a probability: the row stays as it is
                    row = rows[i]
                    row['solution_mass'] = float(mass[k])
                    row['solution_mass_log2'] = float(np.log2(mass[k])) if mass[k] > 0 else None
                    row['solution_mass_open'] = float(open_mass[k])
                    row['solution_mass_proved'] = int(st[k] == 1)
                    if mass[k] > 0:
                        row['posterior'] = posterior[k].tolist()
                    row['mass_work'] = int(zwork[k])
                    if zdepth[k] > 0:
                        row['mass_split_depth'] = int(zdepth[k])
                if hasattr(self, '_mass_stats'):
                    self._mass_stats[0] += int((st == 1).sum()); self._mass_stats[1] += len(sat_rows)
        if self._config.get('complete_nearest'):
            # the satisfiable rows, once more, as one batch of their own: how far PDP's assignment was from a model, and from which one
            from pdp import exact
            sat_rows = [i for i in range(len(rows)) if status[i] == 1]
            if sat_rows:
                items = exact.items_of(graph_map, batch_variable_map, batch_function_map, edge_feature, len(rows))
                pred = hint.cpu().numpy()
                # config['complete_nearest_split']: the search of every row spread over 2^depth waves (pdp_exact_nearest_split); -1: auto.
                # The model the complete search has just found is the start model: the cubes look below its distance only.
                nsplit = self._config.get('complete_nearest_split')
                nsplit = None if nsplit is None else ('auto' if int(nsplit) < 0 else int(nsplit))
                # config['complete_nearest_rounds']: the same search in rounds of 2^N reads per cube (pdp_exact_nearest_round); -1: the default
                nrounds = self._config.get('complete_nearest_rounds')
                begin = None if nsplit is None and nrounds is None else [np.asarray(rows[i]['solution'], dtype=np.float32) for i in sat_rows]
                near, nhints = [items[i] for i in sat_rows], [pred[offs[i]:offs[i + 1]] for i in sat_rows]
                if nrounds is not None:
                    st, cost, models, nwork, ndepth = exact.nearest_model_rounds(near, nhints, budget=budget, device=hint.device, start=begin,
                                                                                 round_budget=None if int(nrounds) < 0 else 1 << int(nrounds),
                                                                                 depths=True)
                else:
                    st, cost, models, nwork, ndepth = exact.nearest_model(near, nhints, budget=budget, device=hint.device, split=nsplit,
                                                                          start=begin, depths=True)
                for k, i in enumerate(sat_rows):
                    row = rows[i]
                    if cost[k] >= 0:
                        row['nearest'] = int(cost[k])
                    row['nearest_proved'] = int(st[k] == 1)
                    row['nearest_solution'], row['nearest_work'] = models[k].astype(int).tolist(), int(nwork[k])
                    if nrounds is not None:
                        row['nearest_rounds'] = int(ndepth[k])
                    elif ndepth[k] > 0:
                        row['nearest_split_depth'] = int(ndepth[k])
                if hasattr(self, '_nearest_stats'):
                    self._nearest_stats[0] += int((st == 1).sum()); self._nearest_stats[1] += len(sat_rows)
        if hasattr(self, '_complete_stats'):
            for k, s in enumerate((1, 0, -1)):
                self._complete_stats[k] += int((status == s).sum())
        return self._write_rows(rows)

    def _check_recurrence_termination(self, active, prediction, sat_problem):
        "De-activates the instances the model has already solved (reference: trainer.py:150-162)."
        sat_problem._native.check_termination(active.reshape(-1), prediction[0].reshape(-1).contiguous())

    _check_recurrence_termination._pdp_standard_termination = True
