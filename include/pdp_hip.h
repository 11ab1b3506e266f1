/*
 * pdp_hip.h -- C ABI of the MI355X-native PDP hot path (libpdp_hip.so).
 *
 * The reference (microsoft/PDP-Solver) has no FFI: its hot path is Python calling torch operators.
 * This header is therefore the boundary a maintainer binds (ctypes stub in INTEGRATION.md) in place
 * of those operator call-site groups.  Every entry point names the reference code it replaces.
 * All pointers are DEVICE pointers unless the name ends in `_host`; all arrays are dense,
 * C-contiguous, fp32 / int32 / uint8 / int64 as declared; `stream` is a hipStream_t (may be NULL).
 * Functions return PDP_OK (0) or an error code; pdp_last_error() gives the message.  Unless stated
 * otherwise calls are asynchronous on `stream`.
 *
 * Batch layout (reference: src/pdp/factorgraph/dataset.py:165-187): instance ids in
 * batch_variable_map / batch_function_map are non-decreasing, variable / clause ids are global and
 * contiguous per instance, edges of one instance are contiguous.  Anything else -> PDP_ERR_LAYOUT.
 */
#ifndef PDP_HIP_H
#define PDP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): pdp_train_gru_backward's scratch contract and the training entry points added in round 4; a coupled multi-process forward
 * (pdp_problem_set_exchange) reports PDP_ERR_SPECULATION on EVERY part when one part cannot take the resident loops.
 * pdp_exact_solve, pdp_exact_solve_hinted, pdp_exact_solve_learn, pdp_exact_learn_reductions, pdp_exact_solve_learn_proof, pdp_exact_check,
 * pdp_exact_trim, pdp_exact_solve_learn_assume, pdp_exact_min_unsat, pdp_exact_count, pdp_exact_solve_split, pdp_exact_split_cubes, pdp_exact_count_split, pdp_exact_count_split_cubes, pdp_exact_count_frontier_words, pdp_exact_count_round, pdp_exact_count_expand, pdp_exact_models_at, pdp_exact_min_unsat_split, pdp_exact_min_unsat_split_cubes, pdp_exact_mass, pdp_exact_mass_split, pdp_exact_mass_split_cubes, pdp_exact_nearest, pdp_exact_nearest_split, pdp_exact_nearest_split_cubes and pdp_exact_last_grid are additions that change no existing entry point or structure, so the version stays 3. */
#define PDP_ABI_VERSION 3

enum {
    PDP_OK = 0,
    PDP_ERR_INVALID = 1,      /* bad argument */
    PDP_ERR_LAYOUT = 2,       /* batch not in the loader's instance-contiguous layout */
    PDP_ERR_HIP = 3,          /* HIP runtime error (no device, OOM, launch failure) */
    PDP_ERR_UNSUPPORTED = 4,
    PDP_ERR_SPECULATION = 5   /* persistent solve hit a cross-instance coupling; rerun step-wise */
};

enum { PDP_RNG_STREAM = 0, PDP_RNG_PHILOX = 1 };
enum { PDP_MODEL_SP = 0, PDP_MODEL_WALKSAT = 1, PDP_MODEL_REINFORCE = 2 };

typedef struct pdp_problem pdp_problem;       /* a batch of CNF instances resident in HBM */
typedef struct pdp_decimator pdp_decimator;   /* SequentialDecimator / ReinforceDecimator state */

int pdp_abi_version(void);
const char *pdp_last_error(void);
int pdp_device_count(void);

/* ---- problem container --------------------------------------------------------------------
 * replaces: SATProblem.__init__/setup_problem, the 24 sparse COO masks and _replicate_batch
 * (reference: src/pdp/nn/solver.py:22-178).  graph_map is [2,E] (row 0 variable id, row 1 clause
 * id), edge_feature [E] in {-1,+1}.  With replication R > 1 the handle holds R copies laid out as
 * solver.py:56-82 does (replica r of instance i has id i + r*B).  Synchronous. */
int pdp_problem_create(pdp_problem **out, int E, int V, int F, int B, int replication,
                       const int32_t *graph_map, const int32_t *batch_variable_map,
                       const int32_t *batch_function_map, const float *edge_feature, void *stream);
int pdp_problem_destroy(pdp_problem *p);
/* dims_host[8] = {E, V, F, B, R, max_vars, max_clauses, max_edges} of the (replicated) batch */
int pdp_problem_dims(const pdp_problem *p, int32_t *dims_host);
/* replicated graph arrays for the Python-visible attributes (_graph_map ...); any may be NULL */
int pdp_problem_export_graph(const pdp_problem *p, int32_t *graph_map, int32_t *batch_variable_map,
                             int32_t *batch_function_map, float *edge_feature, void *stream);
/* binds caller-owned state tensors: _active_variables [V], _active_functions [F], _solution [V],
 * _is_sat [B], _edge_mask [E] (reference: solver.py:49-54,370) and initialises them (1, 1, 0.5, 0.5, 1) */
int pdp_problem_bind_state(pdp_problem *p, float *active_variables, float *active_functions,
                           float *solution, float *is_sat, float *edge_mask, void *stream);

/* ---- K7: simplification ---------------------------------------------------------------------
 * replaces: SATProblem.simplify/_propagate_single_clauses/_peel (solver.py:180-203,228-285) */
int pdp_simplify(pdp_problem *p, void *stream);
/* replaces: SATProblem.set_variables/_set_variable_core (solver.py:205-226,275-279);
 * assignment [V] in {-1,0,+1} is masked in place by the active flags like the reference does */
int pdp_set_variables(pdp_problem *p, float *assignment, void *stream);
/* K8 replaces: solver.py:370-371 / 439-440.  Writes the bound _edge_mask; if all_active_host is
 * non-NULL the call synchronises and stores 1 when every edge is still active, else 0. */
int pdp_refresh_edge_mask(pdp_problem *p, int32_t *all_active_host, void *stream);

/* ---- K4 / K5 ----------------------------------------------------------------------------------
 * replaces: util.sparse_smooth_max (util.py:282-286) with mask = variable mask: x [E] -> out [V] */
int pdp_smooth_max(pdp_problem *p, const float *x, float *out, void *stream);
/* replaces: util.sparse_max / sparse_argmax (util.py:257-275) with mask = batch-variable mask,
 * including the batch-global `x - x.min() + 1` shift: x [V] -> out [B] */
int pdp_instance_max(pdp_problem *p, const float *x, float *out, void *stream);
int pdp_instance_argmax(pdp_problem *p, const float *x, int64_t *out, void *stream);

/* ---- K1-K3: survey propagation sweep ------------------------------------------------------------
 * replaces: SurveyPropagator.forward (pdp_propagate.py:139-221, include_adaptors=False).
 * dec_q [E,3], dec_fs [E,2] = decimator_state; edge_mask [E] or NULL; active_mask uint8 [B] or NULL;
 * init_q / init_fs = init_state; outputs out_q [E,3], out_fs [E,2] (may not alias the inputs). */
int pdp_sp_propagate(pdp_problem *p, const float *dec_q, const float *dec_fs, const float *edge_mask,
                     const uint8_t *active_mask, const float *init_q, const float *init_fs, float pi,
                     float *out_q, float *out_fs, void *stream);

/* ---- adaptor form of the propagator (model type p-nd-np) ------------------------------------------
 * replaces: the include_adaptors=True branches of SurveyPropagator.forward (pdp_propagate.py:166-167, 179-182).
 * dec_v / dec_f [E,H] = neural decimator state; w_f [H] = _function_input_projector.weight, W_v [2,H] =
 * _variable_input_projector.weight; outputs xlog [E] = logsigmoid(w_f . dec_v) and fs2 [E,2] =
 * (sigmoid(W_v[0] . dec_f), sign(W_v[1] . dec_f)). */
int pdp_sp_adaptors(pdp_problem *p, int H, const float *dec_v, const float *dec_f, const float *w_f, const float *W_v,
                    float *xlog, float *fs2, void *stream);
/* pdp_sp_propagate with the clause-to-variable input already in the log domain (xlog [E] from pdp_sp_adaptors) */
int pdp_sp_propagate_adapted(pdp_problem *p, const float *xlog, const float *dec_fs, const float *edge_mask,
                             const uint8_t *active_mask, const float *init_q, const float *init_fs, float pi,
                             float *out_q, float *out_fs, void *stream);
/* K6 replaces: SurveyScorer.forward (pdp_predict.py:155-192): fs [E,2] -> score [V] */
int pdp_survey_score(pdp_problem *p, const float *fs, float pi, float *score, void *stream);

/* ---- K9 / K13 -------------------------------------------------------------------------------------
 * replaces: SatCNFEvaluator.forward (util.py:210-236): pred [V] -> solved [B], unsat_clauses [B] */
int pdp_cnf_eval(pdp_problem *p, const float *pred, float *solved, float *unsat, void *stream);

/* replaces: SatLossEvaluator.forward (util.py:178-197), the energy loss of a prediction reported by the test mode
 * (trainer.py:108-123, base.py:223-250).  pred [V]; coeff = min(global_step^exploration, max_coeff) (host); loss_sharpness a
 * positive integer; loss: device float [1] = mean over the clauses of the batch. */
int pdp_sat_loss(pdp_problem *p, const float *pred, float coeff, float eps, int sharpness, float *loss, void *stream);
/* replaces: PropagatorDecimatorSolverBase._update_solution (solver.py:388-399): out [V] */
int pdp_update_solution(pdp_problem *p, const float *pred, float *out, void *stream);
/* replaces: SatFactorGraphTrainer._check_recurrence_termination (trainer.py:150-162), replication aware */
int pdp_check_termination(pdp_problem *p, uint8_t *active_mask, const float *pred, void *stream);
/* replaces: the per-sweep host read that ends the plug-in loop, `if int(active_mask.sum()) <= 0: break` (solver.py:383-384), for callers that
 * enqueue the sweeps of a forward without waiting for them (the neural triples: one captured HIP graph per sweep parity, pdp/nn/solver.py).
 * pdp_loop_begin clears the loop's two device words; pdp_loop_step, enqueued behind a sweep's termination check, counts the sweep and raises
 * the stop word when no instance of active_mask [B] is active any more (active_mask NULL: no termination check, it only counts); behind
 * the stop word the operators that write message states under an active mask (pdp_neural_aggregate_edges, pdp_neural_gru,
 * pdp_sp_propagate / _adapted) enqueue kernels that return at once, so sweeps already in flight change nothing; pdp_loop_read waits for
 * the stream and returns the stop word and the executed sweeps (= the reference's iteration count), and with end != 0 clears both words. */
int pdp_loop_begin(pdp_problem *p, void *stream);
int pdp_loop_step(pdp_problem *p, const uint8_t *active_mask, void *stream);
int pdp_loop_read(pdp_problem *p, int32_t *stopped_host, int32_t *iterations_host, int end, void *stream);

/* ---- decimators --------------------------------------------------------------------------------------
 * replaces: SequentialDecimator state (_previous_function_state, _counters; pdp_decimate.py:115-125,179-183) */
int pdp_decimator_create(pdp_decimator **out, pdp_problem *p);
int pdp_decimator_destroy(pdp_decimator *d);
int pdp_decimator_reset(pdp_decimator *d, void *stream);
/* replaces: SequentialDecimator.forward with scorer = SurveyScorer (pdp_decimate.py:122-177) */
int pdp_sequential_decimate(pdp_problem *p, pdp_decimator *d, const float *fs, uint8_t *active_mask,
                            float tolerance, float t_max, float pi, void *stream);
/* the same in two halves for a non-native scorer plug-in: gate = :124-150 (returns via
 * any_converged_host, synchronises), apply = :156-173 with a caller-computed score [V] */
int pdp_sequential_decimate_gate(pdp_problem *p, pdp_decimator *d, const float *fs, uint8_t *active_mask,
                                 float tolerance, float t_max, int32_t *any_converged_host, void *stream);
int pdp_sequential_decimate_apply(pdp_problem *p, pdp_decimator *d, const float *fs, const float *score,
                                  const uint8_t *active_mask, void *stream);
/* replaces: ReinforceDecimator.forward (pdp_decimate.py:202-234); fs [E,2] updated in place; coin =
 * the caller's torch.rand(1) draw */
int pdp_reinforce_decimate(pdp_problem *p, pdp_decimator *d, float *fs, uint8_t *active_mask, float coin,
                           float decimation_probability, float pi, void *stream);
/* replaces: ReinforcePredictor.forward (pdp_predict.py:221-226): fs [E,2] -> pred [V] */
int pdp_reinforce_predict(pdp_problem *p, const float *fs, float *pred, void *stream);

/* ---- K14: Walk-SAT ------------------------------------------------------------------------------------
 * replaces: _compute_energy (solver.py:486-496): assignment [V] -> energy [B], unsat_functions [F] */
int pdp_energy(pdp_problem *p, const float *assignment, float *energy, float *unsat_functions, void *stream);
/* replaces: _compute_energy_diff (solver.py:469-484) using the bound _edge_mask: -> delta [V] */
int pdp_energy_diff(pdp_problem *p, const float *assignment, float *delta, void *stream);
/* The in-kernel (PDP_RNG_PHILOX) draws of pdp_random_fill / pdp_local_search are Philox counters of the variable's / the instance's index
 * inside the forward (pdp_predict.py:125-126 draws rand(n_active), solver.py:457,460 rand(V,1) and rand(B): one number per variable /
 * instance of the batch).  When the batch of this problem is a contiguous PART of a larger forward solved elsewhere (isolated instances
 * dealt to several GPUs, pdp/parallel.py) the caller states where the part starts: the draws are then those of the whole forward.
 * Replication 1 only.  Default 0, 0. */
int pdp_problem_set_rng_base(pdp_problem *p, uint32_t first_variable, uint32_t first_instance);
/* One COUPLED forward solved by several processes (one per GPU), each holding a contiguous part of the batch (pdp_problem_set_rng_base says
 * where).  The reference couples the instances of a forward through batch-wide reductions -- the first sweep with a NaN survey (it stops the
 * decimation of the whole batch), the exact zero inside util.sparse_max / sparse_argmax's x - min(x) + 1, the executed sweeps, and the same
 * zero in every Walk-SAT step.  The chunked LDS-resident solver (pdp_sp_solve) and the persistent Walk-SAT
 * (pdp_local_search) take these from a few control words per chunk; with a callback set they hand those words to it between the launches and
 * continue with what it returns: fn(user, mins, n_mins, maxs, n_maxs, ors, n_ors) replaces every element by its minimum / maximum /
 * bit-wise OR over all parts, in place (host memory), and returns 0.  Every part calls it the same number of times (the control flow depends
 * on the merged words only).  Restrictions: SP triple, no batch replication, every instance of a part fits the LDS-resident solver; a failed
 * speculation cannot fall back to the step-wise loop across processes: PDP_ERR_SPECULATION / PDP_ERR_UNSUPPORTED go to the caller.
 * NULL removes the callback. */
typedef int (*pdp_exchange_fn)(void *user, uint32_t *mins, int n_mins, uint32_t *maxs, int n_maxs, uint32_t *ors, int n_ors);
int pdp_problem_set_exchange(pdp_problem *p, pdp_exchange_fn fn, void *user);
/* replaces: IdentityPredictor.forward(last_call=True) random fill (pdp_predict.py:121-126).
 * PDP_RNG_STREAM: values [n_active] are consumed in variable order; PDP_RNG_PHILOX: in-kernel. */
int pdp_random_fill(pdp_problem *p, int rng_mode, const float *values, uint64_t seed, void *stream);
/* replaces: PropagatorDecimatorSolverBase._local_search (solver.py:433-467).  pred [V] -> out [V].
 * PDP_RNG_STREAM: var_rand [iterations,V] and coin_rand [iterations,B] hold the torch.rand draws of
 * each step.  Synchronises; steps_host receives the number of executed steps (global early exit).
 * All steps run in one persistent launch per instance (LDS-resident, or an HBM-resident form for instances past
 * the LDS limit, routed per instance); the strict three-launches-per-step loop is the fallback. */
int pdp_local_search(pdp_problem *p, const float *pred, int iterations, float epsilon, int rng_mode,
                     const float *var_rand, const float *coin_rand, uint64_t seed, float *out,
                     int32_t *steps_host, void *stream);
/* replaces: _deduplicate (solver.py:401-431, with the integer-division fix): pred [V] -> out [V/R],
 * chosen replica per original instance [B/R] (may be NULL) */
int pdp_deduplicate(pdp_problem *p, const float *pred, float *out, int32_t *chosen, void *stream);

/* ---- batched complete solver ---------------------------------------------------------------------------
 * replaces: the reference's labelling hook is_sat (src/pdp/generator.py:15-17, "invoke your SAT solver of choice"), which PDP itself
 * cannot fill: PDP is incomplete and never proves an instance unsatisfiable.  DPLL with unit propagation and chronological backtracking,
 * no clause learning, one wave per instance ("Complete solver").
 * Reads the topology only (instance offsets, e_var / e_sgn in clause order); bound state, simplify(), decimation and edge masks are
 * ignored.  Any instance the layout holds is accepted (unit, empty and tautological clauses, repeated literals, variables without
 * occurrences, instances without clauses); small instances run from LDS, the others from HBM working arrays (routing decided once per
 * problem from the instance sizes: the only host synchronisation).  A replicated problem (R > 1) -> PDP_ERR_UNSUPPORTED.
 * Outputs: status [B] = 1 satisfiable, 0 unsatisfiable, -1 undecided within the budget; model [V] (0 / 1) satisfies every clause of each
 * status-1 instance and is 0 elsewhere (also for variables the search never had to assign); work [B] (may be NULL) = clause-literal reads.
 * budget: clause-literal reads per instance, checked before every unit-propagation pass; an instance stops with -1 at the first check
 * with work >= budget, so work < budget + 3 * (edges of the instance) (a pass reads at most every literal once, the branching scan after it
 * at most twice).  budget <= 0 means PDP_EXACT_DEFAULT_BUDGET.
 * Deterministic and instance-local: status, model and work of an instance do not depend on the batch around it, its position, the call
 * or the library build.  Asynchronous on `stream`; calls on one problem must not overlap (they share its working arrays). */
#define PDP_EXACT_DEFAULT_BUDGET (((int64_t)1) << 32)
int pdp_exact_solve(pdp_problem *p, int64_t budget, int8_t *status, float *model, int64_t *work, void *stream);

/* The same search with phase hints: an assignment that violates few clauses (a PDP prediction) steers the search towards itself.
 * hint [V], one float per variable in the problem's variable order: h > 0.5 = "true first", any other finite value = "false first",
 * NaN = "no hint for this variable" (the reference's poisoning leaves NaN predictions).  hint == NULL behaves as all-NaN.
 * For one instance the search is pdp_exact_solve's with two additions:
 *   1. Check pass, only if none of the instance's hints is NaN: every clause is read up to and including its first literal that is true
 *      under the thresholded hint, and these reads count into work.  If every clause has such a literal the instance is done: status 1,
 *      model[v] = (h[v] > 0.5) for all of its variables, work = the reads of this pass.  Otherwise the search starts from the empty
 *      assignment as in pdp_exact_solve, keeping the reads already counted.  An instance with a NaN hint skips the pass and reads nothing.
 *   2. Polarity: at a decision on variable v the first polarity is the hint's when h[v] is not NaN, else pdp_exact_solve's (true when
 *      its occurrences are at least as many).  The choice of v and everything else are unchanged.
 * The budget is checked where pdp_exact_solve checks it; the check pass runs before the first check, at work = 0, and reads at most every
 * literal once, so work < budget + 3 * (edges of the instance) holds as before.  Status, model and work are a function of the instance
 * and its own hints only.  Consequences: hints never change the status of a search that runs to its end; an unsatisfiable instance's work
 * is pdp_exact_solve's plus the check-pass reads; with pdp_exact_solve's model as the hint the check pass accepts it and work is at most
 * pdp_exact_solve's; all-NaN hints give pdp_exact_solve's three outputs exactly.  R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules. */
int pdp_exact_solve_hinted(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, float *model, int64_t *work, void *stream);

/* The same search with conflict clause learning and backjumping instead of chronological backtracking (opt-in: the two entry points above
 * are unchanged).  hint as in pdp_exact_solve_hinted (may be NULL); arena = 16-bit-word budget for learned clauses per instance (a clause
 * of len literals takes len + 1 words), 0 = four words per literal (edge) of the instance, at most 2^30; learned [B] (may be NULL) = the
 * clauses learned per instance, deleted ones included.  Literal coding, the pass structure (a clause stops reading at its first true
 * literal, units are applied at the end of the pass), the branching rule, hint codes, the check pass, the budget check before every pass
 * and work = clause-literal reads are pdp_exact_solve_hinted's.  New per instance: lev[v], the decision level of an assigned variable,
 * rsn[v], the clause that implied it (none for a decision), and the learned clauses, which get the indices m, m + 1, ... in learning
 * order and take part in every pass and every branching scan after the original ones.
 *   Propagation pass over all live clauses in ascending index.  A clause with no true and no unassigned literal is falsified; the conflict
 *     clause is the lowest-index one, and the pending units of that pass are dropped.  Otherwise a unit clause on literal (v, pol) records
 *     the lowest clause index asking for (v, pol).  At the end of the pass let v* be the lowest variable asked for in both polarities, if
 *     any: v* becomes true with its positive request's clause as reason, and its negative request's clause is the conflict clause; other
 *     both-polarity variables stay unassigned.  Every single-polarity variable is assigned with its clause as reason.  All of them enter
 *     the trail in ascending variable order at the current level.
 *   Conflict at level 0: status 0.  Otherwise first-UIP analysis: start from the conflict clause and resolve backwards along the trail
 *     with the reason of the latest seen current-level variable until exactly one current-level literal (the UIP) is left; literals
 *     assigned at level 0 are dropped; work grows by the length of the conflict clause and of every reason resolved with.  The learned
 *     clause is [not UIP, then the remaining literals ascending by variable]; the backjump level bl is the highest level among the
 *     remaining literals (0 if none); every assignment above bl is undone, level = bl, then the clause is stored.  It is not asserted: the
 *     next pass finds it unit.
 *   Arena: if used + len + 1 > arena after the backjump, every learned clause that is not the reason of an assigned variable is deleted,
 *     the others keep their order and are renumbered.  If the clause still does not fit: status -1 with the work so far.
 * Per loop iteration the work added is at most one pass, one scan (twice a pass) and one analysis (every live literal at most once), so
 * work < budget + 4 * (e + arena) for every instance (e = its edges).  Status, model, work and learned are a function of the instance,
 * its hints, the budget and the arena size alone: the same alone, at any batch position, on repeated calls and in both library builds.
 * All-NaN hints equal hint == NULL.  R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules; the routing and the HBM route's arenas are
 * prepared once per problem and arena size (a call with another arena size synchronises the device and rebuilds them). */
int pdp_exact_solve_learn(pdp_problem *p, const float *hint, int64_t budget, int64_t arena, int8_t *status, float *model, int64_t *work,
                          int32_t *learned, void *stream);
/* reductions [B] (device) = how often each instance's arena was reduced in the last pdp_exact_solve_learn call on the problem, ordered
 * after it on `stream`; PDP_ERR_INVALID before the first such call.  A function of the same inputs as the other outputs. */
int pdp_exact_learn_reductions(pdp_problem *p, int32_t *reductions, void *stream);

/* pdp_exact_solve_learn with its lemma log: the evidence for a status 0.  The search is pdp_exact_solve_learn's -- status, model, work,
 * learned and the reductions are that call's for the same inputs; logging reads nothing and decides nothing.  Every learned clause follows
 * by unit propagation from the clauses before it, so the learned clauses in order, ending in the level-0 conflict, are a DRAT-style proof.
 * proof_off [B+1] (device, ascending, >= 0) gives instance b the region proof[proof_off[b] .. proof_off[b+1]) of int32 words.  Whenever a
 * learned clause is stored in the arena, the same literals in the same order (the negated UIP, then the other variables ascending) are
 * appended to the region as one lemma: len, lit_0 .. lit_{len-1}, literal code (v << 1) | negative with the instance-local v.  A clause
 * that does not fit the arena even after a reduction (status -1) is not logged; arena reductions log nothing (a forward check may keep
 * deleted lemmas).  proof_len [B] = the words the instance's lemmas need, counted whether they were written or not.  A lemma is written
 * only if it fits the region completely, and once one does not fit nothing more is written for that instance: the proof of b is complete
 * iff proof_len[b] <= proof_off[b+1] - proof_off[b], and the words of the region past the stored lemmas are not touched.
 * proof == NULL writes nothing (a sizing call; give regions of no words).  An instance answered by the check pass has proof_len 0.
 * proof and proof_len are, like the other outputs, a function of the instance, its hints, the budget and the arena size alone. */
int pdp_exact_solve_learn_proof(pdp_problem *p, const float *hint, int64_t budget, int64_t arena, int8_t *status, float *model, int64_t *work,
                                int32_t *learned, const int64_t *proof_off, int32_t *proof, int64_t *proof_len, void *stream);

/* The check of what a complete search answered, one wave per instance, independent of the searches (plain Python:
 * tests/exact_proof_model.py).  verdict [B]: 1 the answer is proven, 0 it is refuted, -1 not judged; fail_at [B]; work [B] (may be NULL) =
 * clause-literal reads, a clause or lemma being read up to and including its first true literal.
 *   status 1: every clause is read under model (true: > 0.5).  Every clause has a true literal: verdict 1, fail_at -1; otherwise verdict 0
 *     and fail_at = the lowest clause without one.  Every clause is read either way.
 *   status 0: the first proof_len[b] words of the region are lemmas 0 .. L-1.  For i = 0 .. L-1 and then for the empty clause (i = L):
 *     start from the empty assignment; falsify every literal of lemma i (work += len_i; a lemma with both polarities of a variable is
 *     accepted at once); then passes to a fixed point.  Before each pass: work >= budget -> verdict -1, fail_at -1 (budget <= 0 means
 *     PDP_EXACT_DEFAULT_BUDGET).  A pass reads the original clauses, then lemmas 0 .. i-1: a clause with no true and no unassigned literal
 *     is a conflict, one with no true literal whose unassigned literals are all the same literal asks for that literal; the requests are
 *     applied after the pass.  A conflict, or a variable asked for in both polarities: lemma i is accepted.  Neither a conflict nor a
 *     request: verdict 0, fail_at i.  All of 0 .. L accepted: verdict 1, fail_at -1.
 *     The proof is untrusted: before lemma i is used its length must be >= 0 and fit the proof_len[b] words, and every variable id must
 *     be below n; otherwise verdict 0, fail_at i.  Nothing is read outside the region or the instance's arrays.
 *   any other status, or proof_len[b] negative or larger than the region: verdict -1, fail_at -1, work 0, nothing is read.
 * Between two budget checks lie at most one pass and one lemma's own literals: work < budget + e + W (W = the region's words).  Passes read
 * a consistent assignment and every reduction is an OR or a sum, so verdict, fail_at and work are a function of the instance and its
 * proof alone: the same in any batch, at any position and in both library builds.  proof may be NULL if every region is empty.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules; routing and working arrays are prepared once per problem. */
int pdp_exact_check(pdp_problem *p, const int8_t *status, const float *model, const int64_t *proof_off, const int32_t *proof,
                    const int64_t *proof_len, int64_t budget, int8_t *verdict, int32_t *fail_at, int64_t *work, void *stream);

/* The backward check of a proof of unsatisfiability, one wave per instance (plain Python: tests/exact_trim_model.py): which original clauses
 * (the core) and which lemmas the refutation rests on.  proof, proof_off and proof_len are pdp_exact_check's.  Outputs: verdict [B],
 * fail_at [B], work [B] (may be NULL) as there; core [F], one byte per clause in the problem's clause order; keep, one byte per proof word
 * at the offsets of proof; n_core [B] and n_keep [B] (may be NULL), the core clauses and the kept lemmas of each instance.
 *   Only status[b] == 0 is judged (a model needs no core).  Any other status, or proof_len[b] negative, larger than the region, or so
 *   large that clauses + proof_len[b] >= 2^31: verdict -1, fail_at -1, work 0; nothing of the proof is read and keep is not touched.
 *   core is written for every clause of every instance, 0 unless stated otherwise below.
 *   Step 1.  The first proof_len[b] words are parsed into lemmas 0 .. L-1 and ALL of them are validated before one is used: a length must
 *     be >= 0 and fit the proof_len[b] words, every variable id must be below n.  Lemma i the first malformed one: verdict 0, fail_at i,
 *     work 0.  (pdp_exact_check meets a malformed lemma only when it arrives there, and has counted the reads up to it.)
 *   Step 2.  The empty clause i = L is marked.  For i = L down to 0, lemma i is skipped unless it is marked; otherwise the assignment is
 *     cleared, the literals of lemma i are falsified (work += len_i) and passes run to a fixed point.  Before each pass: work >= budget ->
 *     verdict -1, fail_at -1 (budget <= 0 means PDP_EXACT_DEFAULT_BUDGET).  A pass reads the original clauses and then lemmas 0 .. i-1
 *     in ascending index (lemma j has clause index m + j), each up to and including its first true literal, and records the lowest
 *     falsified clause and, per requested literal, the lowest clause that asks for it.  A falsified clause: the antecedents start as
 *     {that clause}.  Otherwise a variable asked for in both polarities: they start as {the positive request's clause, the negative
 *     request's clause} of the lowest such variable, and nothing is assigned.  Otherwise no request: verdict 0, fail_at i.  Otherwise
 *     every request is applied with its clause as the variable's reason, and the next pass runs.
 *     The closure of a start set: every clause of it is marked, and for every literal of a marked clause the reason of its variable, if a
 *     request of this lemma's check assigned it (the lemma's own falsified literals have none), until nothing new is marked.  Each clause
 *     marked in a closure adds its length to work, once per lemma check.  A marked original clause sets its core byte, a marked lemma j
 *     is marked for the backward loop.
 *     (pdp_exact_check accepts a lemma with both polarities of a variable at once.  Here that rule has no counterpart: such a lemma is
 *     never falsified and never asks for a literal, so nothing marks it and it is never checked.)
 *   All marked lemmas refuted: verdict 1, fail_at -1, core as marked, keep = 1 on every word of a marked lemma (its length word and its
 *     literals) and 0 on every other word among the first proof_len[b]; n_core and n_keep count them.  With verdict 0 or -1 the instance's
 *     core bytes and its first proof_len[b] keep bytes are 0, n_core and n_keep are 0.  Words of a region past proof_len[b] are never touched.
 * Between two budget checks lie at most one pass, one closure and one lemma's own literals: work < budget + 3 (e + W), W = the region's
 * words.  Every quantity is a minimum, an OR or a sum over a consistent assignment and the closure is a set, so all seven outputs are a
 * function of the instance and its proof alone: the same in any batch, at any position, at any grid and in both library builds.
 * Consequences (unit propagation is monotone, and a check that needs fewer lemmas has fewer to refute):
 *   T1  pdp_exact_check verdict 1 on a proof implies pdp_exact_trim verdict 1 on it.
 *   T2  pdp_exact_trim verdict 0 implies pdp_exact_check verdict 0.
 *   T3  with verdict 1, the clauses with core = 1 are unsatisfiable on their own;
 *   T4  with verdict 1, the kept lemmas in order are a proof that pdp_exact_check accepts against those clauses alone.
 * T3 and T4 hold for ANY input words -- genuine, mutated or forged: every kept lemma was refuted from core clauses and kept lemmas before
 * it.  The backward check may accept a proof the forward check refutes, because a bad lemma nobody needs is never looked at; that is
 * sound (T3), and it is why verdict 0 here is the weaker alarm.  proof and keep may both be NULL if every region is empty.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules; routing and working arrays are prepared once per problem. */
int pdp_exact_trim(pdp_problem *p, const int8_t *status, const int64_t *proof_off, const int32_t *proof, const int64_t *proof_len,
                   int64_t budget, int8_t *verdict, int32_t *fail_at, int64_t *work,
                   int8_t *core, int8_t *keep, int32_t *n_core, int32_t *n_keep, void *stream);

/* pdp_exact_solve_learn under assumptions: is the instance satisfiable with these literals held fixed, and if not, which of them are to
 * blame (plain Python: tests/exact_assume_model.py).  assume [V] (may be NULL = all zero), one int8 per variable in the problem's variable
 * order: > 0 the variable is assumed true, < 0 assumed false, 0 not assumed.  failed [V] (may be NULL): 1 on the variables of the failed
 * set of a status-0 instance, 0 everywhere else.  The other arguments are pdp_exact_solve_learn's, and pdp_exact_learn_reductions reports
 * this call's reductions as well.  The search of one instance is pdp_exact_solve_learn's, with these additions for an instance that has
 * at least one assumed variable:
 *   1. Effective code.  The hint code of an assumed variable is the assumption's polarity, whatever hint[v] says, and everything that reads
 *      the code reads this one: the check pass runs iff no variable is left without a code, the assignment it tests agrees with every
 *      assumption, and a check pass that accepts is a correct status 1.
 *   2. The assumption level.  Level 1 belongs to the assumptions.  It is opened when a pass at level 0 ends with no conflict and no unit
 *      request (the fixed point of level 0), before the "no open clause" test and before any branching scan: level = 1, mark[1] = the trail
 *      length, and the assumed variables are visited in ascending index.  An unassigned one gets its assumed value at level 1 with no
 *      reason and enters the trail (in ascending order); one that level 0 assigned to its assumed value is skipped; if level 0 assigned any
 *      to the opposite value the instance ends with status 0 and failed = {the lowest such variable}.  Opening reads no clause literal, so
 *      work does not move; the loop goes on with the next budget check and pass.  Search decisions therefore start at level 2.  A backjump
 *      to level 0 (a learned clause with no literal above level 0) undoes level 1 like any other level, and the level is opened again at
 *      the next fixed point of level 0.
 *   3. Conflict at level 1: status 0, "unsatisfiable under the assumptions", after the final analysis.  It starts from the conflict clause
 *      and walks the trail backwards like the first-UIP analysis, but down to mark[1] and without stopping at a UIP: a seen level-1
 *      variable with a reason is resolved with it, a seen level-1 variable without a reason is an assumption and goes into failed, level-0
 *      variables are dropped.  work grows by the length of the conflict clause and of every reason resolved with.  No clause is learned
 *      from it and learned does not count it.  A conflict at level 0 stays status 0 with an empty failed: the formula is unsatisfiable on
 *      its own.
 *   4. First-UIP analysis at levels >= 2 is unchanged.  Level-1 literals are "a lower level above 0", so they enter the learned clause:
 *      every learned clause follows from the formula alone, never from the assumptions (the certificate of a status 0 under assumptions
 *      relies on that: the instance plus its failed assumptions as unit clauses goes through pdp_exact_solve_learn_proof as it stands).
 *   5. The budget check, the arena rule and work < budget + 4 * (e + arena) are unchanged: the final analysis reads every live literal at
 *      most once and takes the place of a first-UIP analysis in its iteration.  model of a status-1 instance satisfies every clause and
 *      every assumption.  All six outputs are a function of the instance, its hints, its assumptions, the budget and the arena size alone.
 *   6. An instance with no assumed variable (or assume == NULL) gets pdp_exact_solve_learn's five outputs exactly, and an all-zero failed.
 * Consequences:
 *   A1  item 6.
 *   A2  a status-1 model agrees with the assumptions.
 *   A3  failed is a subset of the assumed variables, and the instance plus the failed assumptions as unit clauses is unsatisfiable.
 *   A4  a decided status equals the status of the instance with all assumptions appended as unit clauses.
 *   A5  assuming every variable at the value of a model gives status 1 with that model from the check pass, and work = that pass's reads.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules; routing, working arrays and arenas are pdp_exact_solve_learn's, shared with it. */
int pdp_exact_solve_learn_assume(pdp_problem *p, const float *hint, const int8_t *assume, int64_t budget, int64_t arena,
                                 int8_t *status, float *model, int64_t *work, int32_t *learned, int8_t *failed, void *stream);

/* The fewest unsatisfied clauses of every instance, by depth-first branch and bound over pdp_exact_solve_hinted's passes (plain Python:
 * tests/exact_min_unsat_model.py).  hint [V] (may be NULL) is the first incumbent: h > 0.5 true, every other value false, NaN
 * included; NULL = all false.  Outputs per instance: status = 1, cost is the minimum number of unsatisfied clauses over all assignments,
 * or -1, the budget ran out and cost is an upper bound (never 0); cost [B] = the clauses model leaves unsatisfied, in both cases; model [V]
 * = a complete 0 / 1 assignment (never a placeholder); work [B] (may be NULL) = clause-literal reads; improvements [B] (may be NULL) = how
 * often the incumbent was replaced.  The search of one instance is pdp_exact_solve_hinted's loop with these changes:
 *   Incumbent.  A check pass over the thresholded hint always runs, before the first budget check: every clause is read up to and
 *      including its first true literal (the whole clause if there is none), counted into work; ub = the clauses without a true literal,
 *      model = that assignment.  ub == 0: done, status 1, cost 0.  Otherwise the search starts from the empty assignment.
 *   A pass computes what pdp_exact_solve's computes, and cost = the clauses with no true and no unassigned literal (there: the conflict
 *      flag), contra = the variables whose unit requests name both polarities, wmin = the minimum width over the clauses with no true and
 *      at least one unassigned literal, where a unit (all unassigned literals the same literal) has width 1.
 *   After the pass, in this order:
 *      1. cost + contra >= ub: prune (of two contradicting units one is falsified, and different variables mean different clauses).
 *      2. else cost == ub - 1 and there is a unit: every unit is forced; the pending set is assigned as in pdp_exact_solve, next pass.
 *      3. else no open clause: a leaf with cost < ub.  ub = cost, improvements + 1, model = the current assignment with the unassigned
 *         variables false; ub == 0 ends the search with status 1, otherwise prune.
 *      4. else the unit requests are dropped and the search branches: pdp_exact_solve's rule over the clauses of width wmin (which may be
 *         1 here), first polarity the incumbent hint's (without hints: false).
 *   Prune is pdp_exact_solve's chronological backtracking; running out of levels ends the search with status 1 and cost = ub.
 * The budget is checked before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET) and work < budget + 3 * (edges of the instance) holds.
 * All five outputs are a function of the instance and its own hints: every reduction is an integer sum, an OR, a minimum or a maximum of
 * unique keys.  M1: if the hint has no NaN and leaves at most one clause unsatisfied, work equals pdp_exact_solve_hinted's with the same
 * hint, and cost is 0 where that search answers 1 and the hint's cost where it answers 0 (with ub = 1 every pass is in case 1 or 2).
 * The bound is cost + contra and nothing stronger: k disjoint unsatisfiable blocks take about 8^k leaves.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules; routing and working arrays are pdp_exact_solve's, shared with it. */
int pdp_exact_min_unsat(pdp_problem *p, const float *hint, int64_t budget, int8_t *status, int32_t *cost, float *model,
                        int64_t *work, int32_t *improvements, void *stream);

/* The model of every instance that is nearest to a hint, by depth-first branch and bound over pdp_exact_solve_hinted's passes with the
 * cost on the variables and every clause hard (plain Python, normative: tests/exact_nearest_model.py).  hint [V] (may be
 * NULL) is the point the distance is measured from: h > 0.5 true, every other value false, NaN included; NULL = all false.  penalty [V]
 * (device int32, may be NULL = all 1) is what a variable costs where the model differs from the hint, an integer in [0, 2^20]:
 * cost(x) = the sum of penalty[v] over the variables with x[v] != hint bit of v, a 64-bit integer; all 1 gives the Hamming distance.
 * Outputs per instance: status = 1, cost is the minimum over the models and model attains it; 0, the instance has no model (cost -1, model
 * all 0); -1, the budget ran out: cost and model are the best model met so far (an upper bound), or -1 and all 0 if none was met; -3, a
 * penalty of the instance is outside [0, 2^20]: it is not searched and cost, model, work and improvements are 0.  cost [B] (int64);
 * model [V] = a complete 0 / 1 assignment wherever cost >= 0; work [B] (may be NULL) = clause-literal reads; improvements [B] (may be NULL)
 * = how often a better model was met.  The search of one instance:
 *   Check pass.  It always runs, before the first budget check, and is pdp_exact_solve_hinted's: every clause is read up to and including
 *      its first literal that is true under the hint (the whole clause if there is none), counted into work.  Every clause has one: status
 *      1, cost 0, model = the hint, improvements 0.  Otherwise the search starts from the empty assignment with ub = infinity, dist = 0.
 *   A pass is pdp_exact_solve's: the conflict flag, the unit requests, wmin over the open clauses that are no units.  The pending set is
 *      assigned as there, and dist grows by penalty[v] for every unit assigned against the hint.
 *   After the pass, in this order:
 *      1. a conflict, a variable asked for in both polarities, or dist >= ub: prune.
 *      2. else units were assigned: next pass.
 *      3. else no open clause: a leaf with dist < ub.  ub = dist, improvements + 1, model = the current assignment with every unassigned
 *         variable at its hint value (these cost nothing); ub == 0 ends the search with status 1, otherwise prune.
 *      4. else branch: pdp_exact_solve's variable (most occurrences in the open clauses of width wmin, ties to the lower index), first
 *         polarity the hint's, which costs nothing.
 *   Prune is pdp_exact_solve's chronological backtracking.  Undoing a level takes what its variables had added off dist; flipping a
 *      decision adds the variable's penalty, and if dist >= ub then, the flipped state is pruned at once, before any pass, and backtracking
 *      goes on with this level.  Running out of levels ends the search: status 1 and cost = ub if a model was met, status 0 otherwise.
 * The budget is checked before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET) and work < budget + 3 * (edges of the instance) holds.
 * dist, ub and every sum are 64-bit integers, uniform over the wave; every reduction is an integer sum, an OR, a minimum or a maximum of
 * unique keys: all five outputs are a function of the instance, its hint, its penalties and the budget alone.
 *   N1  a hint that is a model: status 1, cost 0, model = hint, improvements 0, work = pdp_exact_solve_hinted's with that hint.
 *   N2  run to its end, status is pdp_exact_solve's; model satisfies every clause and cost is the penalty sum of model != hint.
 *   N4  the visited tree is a pruned subtree of pdp_exact_count's (the variable choice does not depend on the polarity order):
 *       work <= pdp_exact_count's work + (edges of the instance) wherever the count completes; the extra term is the check pass.
 *   N6  multiplying every penalty by an integer c > 0 (within 2^20) multiplies cost by c and changes no other output.
 * The bound is dist and nothing stronger: an open clause all of whose remaining literals disagree with the hint is not charged before a
 * pass makes it a unit, so with an uninformative hint the tree is about the count's.  There is no limit on n.
 * R != 1 -> PDP_ERR_UNSUPPORTED; NULL status, cost or model -> PDP_ERR_INVALID.  Same stream rules; routing, LDS slab and working arrays
 * are pdp_exact_solve's, shared with it: the penalty lives in bits 10-31 of the word that holds the hint code, and dist is restored from
 * the trail. */
int pdp_exact_nearest(pdp_problem *p, const float *hint, const int32_t *penalty, int64_t budget, int8_t *status, int64_t *cost,
                      float *model, int64_t *work, int32_t *improvements, void *stream);

/* Exact model counts and per-variable counts of every instance: pdp_exact_solve's search (no hints) that does not stop at the first
 * assignment under which no clause is open (plain Python, normative: tests/exact_count_model.py).  Outputs per instance:
 * status = 1, the search is complete and count [B] is the number of models, or -1, the budget ran out and count covers the part of the
 * tree visited so far (a lower bound), or -2, the instance has more than 1023 variables and is not searched (count, true_count, work and
 * leaves are 0); never 0: an unsatisfiable instance is status 1 with count 0.  true_count [V] = the models among those counted in which
 * the variable is true, 0 <= true_count <= count; work [B] (may be NULL) = clause-literal reads; leaves [B] (may be NULL) = the
 * satisfying cubes met.  n counts every variable of the instance, also one in no clause.  All new arithmetic is IEEE double, in this order:
 *   State.  count = 0.0, leaves = 0; T[v] = F[v] = 0.0; snap[level] per decision level, snap[0] = 0.0.
 *   Opening a level.  snap[level] = count.
 *   Leaf (a pass with no conflict, no unit and no open clause).  count = count + ldexp(1.0, n - trail length), leaves + 1, then continue
 *      exactly as after a conflict.
 *   Undoing a level (every level the backtracking pops, and the level whose decision is about to be flipped).  Before its trail entries
 *      are cleared: d = count - snap[level]; for every u on the level's part of the trail, T[u] += d if u is true, else F[u] += d.  When
 *      the decision is flipped to its second polarity, snap[level] = count again.
 *   End (out of levels: status 1; the budget check fired before a pass: status -1).  Every open level is flushed by the same rule, the
 *      newest first, level 0 (the variables fixed by the first propagation) with d = count; then
 *      true_count[v] = T[v] + (count - T[v] - F[v]) * 0.5.
 * Every addend is a non-negative integer and the partial sums are monotone: if count <= 2^53, then count, T, F and true_count are exact
 * integers (count - T - F is even); above, they are the correctly rounded results of this operation order.  Up to n = 1023, 2^n and every
 * partial sum are finite.  The passes, the branching rule (first polarity the one with at least as many occurrences), the budget check and
 * work < budget + 3 * (edges of the instance) are pdp_exact_solve's.  All five outputs are a function of the instance and the budget alone:
 * count and snap are uniform over the wave, T[u] and F[u] are updated by the one lane that holds u's trail slot, and there is no
 * floating-point reduction across lanes.  Every satisfying cube is visited, with no component decomposition and no caching: an
 * under-constrained instance ends at the budget with a lower bound.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream rules; routing and working arrays are pdp_exact_solve's, shared with it; the LDS slab is
 * pdp_exact_solve's plus 24 n + 8 bytes of the kernel's own for snap, T and F (in HBM on the HBM route, T being true_count itself). */
int pdp_exact_count(pdp_problem *p, int64_t budget, int8_t *status, double *count, double *true_count, int64_t *work, int64_t *leaves,
                    void *stream);

/* The exact solution mass of a soft prediction: Z(p) = the sum over the models x of the instance of prod_v (x_v ? p_v : 1 - p_v), the
 * probability that rounding every variable independently with the predicted probability gives a model (plain Python, normative:
 * tests/exact_mass_model.py).  pdp_exact_count's search with a weight per literal.  weights [V] (device float32, the
 * prediction's own dtype): p_v = (double)weights[v]; the positive literal weighs p_v, the negative one 1.0 - p_v, computed in double
 * wherever it is used; an unassigned variable contributes the factor 1.  Outputs per instance: status = 1, the search is complete and
 * mass [B] = Z, or -1, the budget ran out, mass covers the part of the tree visited so far and open_mass [B] the part not yet visited,
 * or -2, the instance has more than 1023 variables, or -3, one of its weights is NaN or outside [0, 1]; -2 and -3 are not searched and
 * every other output of the instance is 0; never 0: an unsatisfiable instance is status 1 with mass 0.  true_mass [V] = the part of
 * mass with the variable true; work [B] and leaves [B] (each may be NULL) as pdp_exact_count's.  All new arithmetic is IEEE double
 * add, subtract and multiply, in this order:
 *   State.  pdp_exact_count's (Z in the place of count), plus mass = 1.0, the product of the weights of everything on the trail, and
 *      pre[level], mass before the level's decision was applied.
 *   Assigning a pass's pending set.  The new trail entries (in variable order) are taken 64 consecutive ones at a time; a chunk's
 *      weights, 1.0 in the lanes without an entry, are multiplied by the xor butterfly 32, 16, 8, 4, 2, 1 (x = x * x[lane ^ o]; a
 *      multiplication commutes, so every lane ends with the same bits); then mass = mass * chunk, chunks in ascending order.
 *   Zero mass.  Once the pending set is assigned and multiplied in (also in a pass that assigned nothing), mass == 0.0 makes the state
 *      a conflict: no leaf is credited, and backtracking runs as after a conflict.  Weights are at most 1, so a prefix of mass 0 stays
 *      0: the rule, underflow included, changes no bit of mass, true_mass or open_mass; it only lowers work (and leaves of mass 0).
 *   Leaf.  Z = Z + mass, leaves + 1, then as after a conflict.
 *   Decision.  The variable is pdp_exact_count's.  pre[level] = mass, snap[level] = Z; the first polarity is the heavier literal (true
 *      if p_v > 0.5, false if p_v < 0.5, pdp_exact_count's rule at exactly 0.5); then mass = mass * (the decided literal's weight).
 *   Flip.  snap[level] = Z, mass = pre[level] * (the other literal's weight).  If that is 0.0 the flipped state is a conflict at once,
 *      before any pass: backtracking goes on with this level (a subtree without mass is pruned for free, so a 0 / 1 prediction costs
 *      one descent).
 *   Crediting.  pdp_exact_count's rule with d = Z - snap[level], the end flush included.
 *   End.  true_mass[v] = T[v] + (Z - T[v] - F[v]) * p_v.  open_mass = 0.0 at status 1.  At status -1 the budget check fired before a
 *      pass, so the current node is unresolved: sequentially, for the levels 1 .. level in ascending order, a level whose decision is
 *      not yet flipped adds pre[level] * (the untried literal's weight); then open_mass = open_mass + mass.
 * The passes, the budget check before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET), work < budget + 3 * (edges of the instance)
 * and leaves are pdp_exact_count's.  Consequences: the true Z lies in [mass, mass + open_mass] up to rounding; mass never falls as the
 * budget rises; with all weights 0.5 the search is pdp_exact_count's state for state -- mass * 2^n == count, true_mass * 2^n ==
 * true_count, work and leaves are equal; with 0 / 1 weights mass is 1.0 if that assignment is a model and 0.0 if not, and leaves <= 1.
 * Every output is a function of the instance, its weights and the budget alone: mass, Z, snap and pre are uniform over the wave, T[u]
 * and F[u] are updated by the one lane that holds u's trail slot, and there is no atomic and no reduction of doubles across lanes other
 * than the stated butterfly; the default and the fast build give the same bits.
 * NULL weights or outputs (other than work and leaves) -> PDP_ERR_INVALID before any launch; R != 1 -> PDP_ERR_UNSUPPORTED.  Same stream
 * rules; routing and working arrays are pdp_exact_solve's, shared with it; the LDS slab is pdp_exact_solve's plus 40 n + 16 bytes of
 * the kernel's own for snap, pre, T, F and the weights as doubles (at most 40 936 bytes), in HBM on the HBM route, in a block that only
 * this call uses, T being true_mass itself. */
int pdp_exact_mass(pdp_problem *p, const float *weights, int64_t budget, int8_t *status, double *mass, double *true_mass,
                   double *open_mass, int64_t *work, int64_t *leaves, void *stream);

/* pdp_exact_mass with the search of every instance spread over 2^depth[b] waves (plain Python, normative:
 * tests/exact_mass_split_model.py).  Cube `index` of the 2^depth cubes of an instance is pdp_exact_mass's search with the
 * decision of every level L <= depth pinned as in pdp_exact_count_split (bit (index >> (depth - L)) & 1: 0 the polarity the mass search
 * tries first -- the heavier literal, pdp_exact_count's rule at exactly 0.5 --, 1 the other; the level counts as already flipped).
 * pre[L] = mass and snap[L] = Z as at any decision, then mass = mass * (the pinned literal's weight).
 *   A pinned decision of mass 0.  If that product is 0.0 the state is a conflict at once, without a pass and without a budget check
 *      (pdp_exact_mass's flip rule: a pinned "other" polarity is a flip); every open level is pinned then, so the cube ends.
 *   A leaf inside the prefix.  A state without an open clause met with L < depth levels open is reached by every cube that shares those
 *      levels' bits; the cube with index & ((1 << (depth - L)) - 1) == 0 adds mass to Z and 1 to leaves, the others add nothing; either
 *      way the cube backtracks as after a conflict (pdp_exact_count_split's rule).
 *   Open mass.  At cube status -1 the levels not yet flipped add pre[level] * (the untried literal's weight) as in pdp_exact_mass; a
 *      pinned level counts as flipped and adds nothing, its sibling cube owns that half.  The cubes that share a prefix make the same
 *      reads up to a node inside it and run out at the same check, so the current node's mass is added only by the cube that owns the
 *      node: level >= depth, or index & ((1 << (depth - level)) - 1) == 0.
 *   The budget is per cube: own reads >= budget before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET).  The end flush and
 *      true_mass_c[v] = T[v] + (Z_c - T[v] - F[v]) * p_v are pdp_exact_mass's, per cube.
 *   The instance's outputs are sums over its cubes in ASCENDING index, sequentially in double: mass = mass + mass_c, open_mass =
 *   open_mass + open_c, true_mass[v] = true_mass[v] + true_mass_c[v]; work and leaves are integer sums; status 1 if every cube's is 1,
 *   else -1, and then Z lies in [mass, mass + open_mass] up to rounding.  Where every product and sum is exact (weights that are small
 *   dyadic fractions) mass, true_mass and leaves equal pdp_exact_mass's bit for bit at every depth; elsewhere they are the correctly
 *   rounded results of this order and may differ from the plain call's in the last bits.  depth 0 gives pdp_exact_mass's six outputs
 *   exactly.  With all weights 0.5 the cubes are pdp_exact_count_split's, record for record.  work >= pdp_exact_mass's (prefixes are
 *   replayed) and work < cubes * (budget + 3 * edges of the instance).
 *   depth [B] (device int8; NULL: all 0) in 0 .. 16; at most 2^22 cubes per call; the per-cube rows below at most 2^31 bytes; any of them
 *   violated -> PDP_ERR_INVALID, the message names the instance.  An instance on the HBM route and an instance of more than 1023
 *   variables (status -2, one record -2 / 0 / 0 / 0 / 0) have one cube.  An instance with a weight that is NaN or outside [0, 1] keeps
 *   its depth: status -3, every other output 0, and each of its cubes leaves the record -3 / 0 / 0 / 0 / 0.  depth_used [B] (int8, may
 *   be NULL) = the depth each instance was searched at.  work and leaves may be NULL.
 * One wave takes one cube at a time from one counter and runs it to its own end; no word is shared between two cubes and no wave waits
 * for another.  A cube of an instance with depth_used > 0 leaves its record and, unless its mass is 0.0, its row of true_mass_c in
 * [cubes][n_max] doubles on the handle; a second kernel sums records and rows per instance in cube order, one lane per variable.  No
 * double goes through an atomic or, other than pdp_exact_mass's stated butterfly, a reduction across lanes: every output and every
 * record is a function of the instance, its weights, the depth and the budget alone; the default and the fast build give the same bits.
 * NULL weights or outputs (other than work, leaves and depth_used) -> PDP_ERR_INVALID before any launch; R != 1 -> PDP_ERR_UNSUPPORTED.
 * Routing, slab and working arrays are pdp_exact_mass's, shared with it; records and rows are a block of this call's own, so a
 * pdp_exact_count_split call on the same problem does not disturb them.  The call synchronises the stream once (the cube count sizes
 * its records and its grid); the kernels that follow are asynchronous on it. */
int pdp_exact_mass_split(pdp_problem *p, const float *weights, const int8_t *depth, int64_t budget, int8_t *status, double *mass,
                         double *true_mass, double *open_mass, int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream);

/* The per-cube records of the last pdp_exact_mass_split call on the problem that succeeded (PDP_ERR_INVALID before the first, and after
 * a call that was refused): cube_off [B+1] (int64), cube_status [cubes] (1 / -1, -2: more than 1023 variables, -3: a bad weight),
 * cube_mass and cube_open [cubes] (double), cube_work and cube_leaves [cubes], cubes = cube_off[B] = the sum of 2^depth_used.  Device to
 * device, asynchronous on the stream. */
int pdp_exact_mass_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, double *cube_mass, double *cube_open,
                               int64_t *cube_work, int64_t *cube_leaves, void *stream);

/* pdp_exact_solve_hinted with the search of every instance spread over 2^depth[b] waves (plain Python, normative:
 * tests/exact_split_model.py).  The deciding search is a deterministic depth-first tree; a cube is a prefix of it: cube
 * `index` of the 2^depth cubes of an instance is that search, without its check pass, where the decision of every level L <= depth is
 * pinned -- the polarity the search would try first if bit (index >> (depth - L)) & 1 is 0, else the other one -- and the level counts as
 * already flipped, so backtracking pops through it and a cube whose subtree is exhausted answers 0.  A cube that meets a state without
 * an open clause before `depth` levels exist answers 1 with that model.  The cubes partition the tree in the order the plain search walks
 * it, so with a budget that no cube exhausts status and model are pdp_exact_solve_hinted's bit for bit, at every depth.
 *   hint [V] (device; NULL: none) as pdp_exact_solve_hinted.  depth [B] (device int8; NULL: all 0) in 0 .. 16; at most 2^22 cubes per call;
 *   either violated -> PDP_ERR_INVALID, the message names the instance.  An instance on the HBM route is searched at depth 0 (its working
 *   arrays are per instance).  depth_used [B] (int8, may be NULL) = the depth each instance was searched at.
 *   The check pass runs once per instance, in a kernel of its own before the cubes, under pdp_exact_solve_hinted's condition (no hint of
 *   the instance is NaN); if it accepts: status 1, that model, work = its reads, first = -1, and the instance's cubes are not searched
 *   (cube status -2, work 0).  Otherwise its reads count against the budget of EVERY cube of the instance: a cube checks
 *   check reads + its own reads >= budget before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET), as the plain search does.
 *   first [B] (int32, may be NULL) = the lowest cube that answers 1, or -1.  If it exists: status 1, model = that cube's, work = check reads
 *   + the work of cubes 0 .. first.  Else status 0 if every cube answers 0, otherwise -1; model 0; work = check reads + the work of all
 *   cubes.  depth 0 gives pdp_exact_solve_hinted's three outputs exactly (pdp_exact_solve's with hint NULL).
 *   work < cubes * (budget + 3 * edges of the instance).
 * One wave takes one cube at a time from one counter: instance order, within an instance ascending index.  A cube that answers 1 lowers
 * best[b] to its index (one atomic minimum); at every budget check a cube whose index is ABOVE best[b] stops (cube status -2).  A cube
 * never stops because of a higher cube and no wave waits for another, so cubes 0 .. first always run to their own end: status, model, work,
 * first, depth_used and the records of cubes <= first are a function of the instance, its hints, its depth and the budget alone.  The
 * records of cubes above first (which of them stopped, and after how many reads) depend on timing.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Routing and working arrays are pdp_exact_solve's, shared with it.  The call synchronises the stream once
 * (the cube count sizes its records and its grid); the kernels that follow are asynchronous on it. */
int pdp_exact_solve_split(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, float *model,
                          int64_t *work, int32_t *first, int8_t *depth_used, void *stream);

/* The per-cube records of the last pdp_exact_solve_split call on the problem that succeeded (PDP_ERR_INVALID before the first): cube_off
 * [B+1] (int64; instance b owns cubes cube_off[b] .. cube_off[b+1]), cube_status [cubes] (1 / 0 / -1, -2 stopped early or not searched) and
 * cube_work [cubes], cubes = cube_off[B] = the sum of 2^depth_used.  Device to device, asynchronous on the stream. */
int pdp_exact_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int64_t *cube_work, void *stream);

/* pdp_exact_count with the search of every instance spread over 2^depth[b] waves (plain Python, normative:
 * tests/exact_count_split_model.py).  Cube `index` of the 2^depth cubes of an instance is pdp_exact_count's search with the
 * decision of every level L <= depth pinned as in pdp_exact_solve_split (bit (index >> (depth - L)) & 1: 0 the polarity the search tries
 * first, 1 the other; the level counts as already flipped).  The cubes partition the tree, so their counts add.  A leaf met with fewer
 * than `depth` levels open (L < depth) is reached by every cube that shares those levels' bits; it is credited to exactly one of them,
 * the cube with index & ((1 << (depth - L)) - 1) == 0, and the others add nothing to count or leaves; either way the cube backtracks as
 * after a conflict, which ends it (every open level is pinned).  The end flush and true_count_c[v] = T[v] + (count_c - T[v] - F[v]) * 0.5
 * are pdp_exact_count's, per cube.  The budget is per cube: own reads >= budget before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET).
 *   The instance's outputs are sums over its cubes in ASCENDING index: count = count + count_c and true_count[v] = true_count[v] +
 *   true_count_c[v], sequentially in double; work and leaves are integer sums; status 1 if every cube's is 1, else -1 (count is then a
 *   lower bound).  While count <= 2^53 every per-cube value is an exact integer and count, true_count and leaves equal pdp_exact_count's
 *   bit for bit at every depth; above, they are the correctly rounded results of this order.  depth 0 gives pdp_exact_count's five
 *   outputs exactly.  work >= pdp_exact_count's (prefixes are replayed) and work < cubes * (budget + 3 * edges of the instance).
 *   depth [B] (device int8; NULL: all 0) in 0 .. 16; at most 2^22 cubes per call; the per-cube rows below at most 2^31 bytes; any of them
 *   violated -> PDP_ERR_INVALID, the message names the instance (for the two sizes: the one at which the running total passes the cap).
 *   An instance on the HBM route and an instance of more than 1023 variables (status -2, one record -2 / 0 / 0 / 0) have one cube;
 *   depth_used [B] (int8, may be NULL) = the depth each instance was searched at.  work and leaves may be NULL.
 * One wave takes one cube at a time from one counter and runs it to its own end; no word is shared between two cubes and no wave waits
 * for another.  A cube of an instance with depth_used > 0 leaves its record and, unless its count is 0.0, its row of true_count_c in
 * [cubes][n_max] doubles on the handle (n_max over those instances); a second kernel sums records and rows per instance in cube order,
 * one lane per variable.  No double goes through an atomic or a reduction across lanes or waves: every output and every record is a
 * function of the instance, the depth and the budget alone.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Routing, slab and working arrays are pdp_exact_count's, shared with it.  The call synchronises the stream
 * once (the cube count sizes its records and its grid); the kernels that follow are asynchronous on it. */
int pdp_exact_count_split(pdp_problem *p, const int8_t *depth, int64_t budget, int8_t *status, double *count, double *true_count,
                          int64_t *work, int64_t *leaves, int8_t *depth_used, void *stream);

/* The per-cube records of the last pdp_exact_count_split call on the problem that succeeded (PDP_ERR_INVALID before the first): cube_off
 * [B+1] (int64), cube_status [cubes] (1 / -1, -2: more than 1023 variables), cube_count [cubes] (double), cube_work and cube_leaves [cubes],
 * cubes = cube_off[B] = the sum of 2^depth_used.  Device to device, asynchronous on the stream. */
int pdp_exact_count_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, double *cube_count, int64_t *cube_work,
                                int64_t *cube_leaves, void *stream);

/* pdp_exact_count as a sequence of short launches ("rounds") that can be stopped, continued and re-cut between launches (plain Python,
 * normative: tests/exact_count_rounds_model.py).  The state of the depth-first search at a budget stop is two bits per
 * decision level: the polarity the level is on, and whether its other polarity is still owed.
 *   Cube.  A cube belongs to one instance and has a path of len levels, 0 <= len <= n.  Level L is bit (L - 1) % 32 of word (L - 1) / 32
 *   of the cube's rows in bits and closed [cubes][words]: (bit, closed) = (0, 0) the polarity the search tries first, the other one
 *   still owed; (0, 1) the first polarity, nothing owed; (1, 1) the other polarity, nothing owed; (1, 0) is refused.  Bits of levels
 *   beyond len are not read.  The root cube has len 0.  pdp_exact_count_split's cube (depth, index) is the path of depth closed levels
 *   with the bits of index.
 *   Search of a cube.  pdp_exact_count's search with plen = len: a decision that opens level L <= plen takes the polarity its bit asks
 *   for (0: the search's own first polarity, 1: the other) and carries the flipped mark iff closed; levels above plen are free.  When
 *   backtracking flips an open level L, plen = min(plen, L): the path beyond a flipped level no longer applies.  A leaf met at a level
 *   < plen is counted iff every path bit of levels level+1 .. plen is 0; either way the search goes on as after a conflict.  snap, the
 *   crediting, the end flush of every open level and true_count_c[v] = T[v] + (count_c - T[v] - F[v]) * 0.5 are pdp_exact_count's.
 *   Budget of a round (reads per cube; budget <= 0: PDP_EXACT_ROUND_BUDGET).  It is tested only where a node begins -- before the first
 *   pass of the cube, of a decision and of a flip -- never between the passes of one propagation.  Reads count against it from the first
 *   node that begins with level >= plen: the replay of the path is free against the budget, but counted in work (cube_replay).  reads
 *   since then >= budget stops the cube with status -1, so every round finishes at least one node beyond its checkpoint, and a cube's
 *   work is at most its replay plus the budget plus one node.
 *   Checkpoint of a stopped cube (len_out, bits_out, closed_out, the same shapes as the inputs and distinct from them): len_out = the open
 *   levels; bit = 1 iff the level is on its other polarity (a path bit, or flipped in this round); closed = its flipped mark.  A cube
 *   that ends (status 1) leaves len_out 0 and a row of zeros.
 *   Accumulation.  Per instance, in ascending cube order: count[b] = count[b] + count_c and true_count[v] = true_count[v] +
 *   true_count_c[v], sequentially in double, INTO the caller's running totals (in/out; zero them before the first round); work[b] and
 *   leaves[b] take integer sums.  No double goes through an atomic or a reduction across lanes.  While the total is <= 2^53 everything is
 *   an exact integer, and a count that runs until its frontier is empty equals pdp_exact_count's count, true_count and leaves bit for bit,
 *   for any budgets and any re-cutting; above, it is the correctly rounded result of this order.
 * pdp_exact_count_frontier_words: *words_host = the words of a path row, max(1, ceil(n_max / 32)) over the instances of at most 1023
 * variables.
 * pdp_exact_count_round: cube_off [B+1] (device int64; instance b owns cubes cube_off[b] .. cube_off[b+1]; cube_off[B] == cubes), len
 * [cubes] (int32), bits / closed [cubes][words].  cube_status [cubes] = 1 / -1.  cube_count (double), cube_work, cube_leaves and
 * cube_replay (int64) [cubes] may be NULL.  A check kernel runs BEFORE anything is searched, and a malformed frontier returns
 * PDP_ERR_INVALID with nothing written, the message naming the cube or instance: cube_off not starting at 0, not monotone or not ending
 * at cubes; len outside 0 .. n; a (1, 0) pair among a path's levels; a cube on an instance of more than 1023 variables (such an instance
 * has no cube; its status is the caller's to keep); more than one cube on an instance of the HBM route (its working arrays are per
 * instance); more than 2^22 cubes, or per-cube rows (cubes x n_max doubles, on the handle) past 2^31 bytes.  One wave takes one cube at a
 * time from one counter; no wave waits for, or reads a word of, another.  The call synchronises the stream once (the check's verdict).
 * pdp_exact_count_expand: from a round's inputs cube_off and outputs cube_status, len_out, bits_out, closed_out, the next frontier.
 * Every stopped cube, in cube order, becomes up to `give` (>= 0) children followed by its remainder: the child of level L is the path of
 * levels 1 .. L-1 with their bits, all closed, followed by (1, 1); children are made for the shallowest min(give, open levels) open
 * levels, in ascending L; the remainder is the checkpoint with those levels closed.  A cube of status 1 leaves nothing.  An instance on
 * the HBM route is never expanded: its one cube is resumed as it is.  The same check runs first (PDP_ERR_INVALID, nothing written); a new
 * frontier of more than `capacity` cubes (the rows of len_new, bits_new and closed_new) or more than 2^22 is refused the same way.
 * *cubes_new_host = the new cube count = cube_off_new[B].  The call synchronises the stream once.
 * Every output of both calls is a function of the instances, the frontier, the budget and give alone.  R != 1 -> PDP_ERR_UNSUPPORTED.
 * Routing, slab and working arrays are pdp_exact_count's, plus T [V] of the HBM route. */
#define PDP_EXACT_ROUND_BUDGET (((int64_t)1) << 18)
int pdp_exact_count_frontier_words(pdp_problem *p, int32_t *words_host);
int pdp_exact_count_round(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int32_t *len, const uint32_t *bits,
                          const uint32_t *closed, int64_t budget, double *count, double *true_count, int64_t *work, int64_t *leaves,
                          int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out, double *cube_count,
                          int64_t *cube_work, int64_t *cube_leaves, int64_t *cube_replay, void *stream);
int pdp_exact_count_expand(pdp_problem *p, const int64_t *cube_off, int64_t cubes, const int8_t *cube_status, const int32_t *len,
                           const uint32_t *bits, const uint32_t *closed, int32_t give, int64_t capacity, int64_t *cube_off_new,
                           int32_t *len_new, uint32_t *bits_new, uint32_t *closed_new, int64_t *cubes_new_host, void *stream);

/* pdp_exact_solve_hinted as a sequence of rounds over the same frontier (plain Python, normative: tests/exact_solve_rounds_model.py;
 * DESIGN.md 9.18).  The frontier (cube_off, len, bits, closed, the pairs, pdp_exact_count_frontier_words), its check and the checkpoints
 * are pdp_exact_count_round's, and the next frontier comes from pdp_exact_count_expand, called as it is with this call's cube_status.
 *   Search of a cube.  pdp_exact_solve_hinted's search without its check pass, with plen = len: a decision that opens level L <= plen takes
 *   the polarity its bit asks for (0: the polarity the search would try first, the hint's where the variable has one; 1: the other) and
 *   carries the flipped mark iff closed.  When backtracking flips an open level L, plen = min(plen, L).  A state without an open clause
 *   answers 1 with that assignment wherever it is met, also at a level < plen: every cube that reaches it holds the same model.  Out of
 *   levels answers 0.  hint [V] may be NULL (no hints).
 *   Budget of a round (reads per cube; budget <= 0: PDP_EXACT_SOLVE_ROUND_BUDGET) and checkpoint: pdp_exact_count_round's, word for word.
 *   A cube of status 0 or 1 leaves len_out 0 and a row of zeros.
 *   Outcome, per instance that has a cube.  first[b] = the lowest cube of the instance, counted from cube_off[b], that answered 1 (-1:
 *   none).  If there is one: status[b] = 1, model (its slice of [V]) = that cube's, and the instance's stopped cubes get cube_status -2
 *   ("dropped"), so that the expansion leaves nothing of them; their checkpoints stay as written.  Else status[b] = 0 if no cube
 *   stopped, else -1.  work[b] (in/out) takes the integer sum of its cubes' work.  An instance without a cube is not touched in status,
 *   model, work or first.  cube_status [cubes] = 1 / 0 / -1 / -2; cube_work and cube_replay [cubes] may be NULL.
 * No word is shared between two cubes: a cube of a satisfiable instance runs out its round even if a sibling has a model already, so
 * every output, record and frontier word is a function of the instances, the hints, the frontier and the budget alone.  With one cube per
 * instance throughout (give 0) status and model are pdp_exact_solve_hinted's bit for bit wherever that call's check pass does not accept
 * the hints, and the sum of cube_work - cube_replay over the rounds is its work less the check pass's reads; with more, which model comes
 * back is not promised.  One wave takes one cube at a time from one counter; a cube that answered 1 leaves its model as a row of bytes in
 * [cubes][n_max] on the handle; a second kernel writes the outcome, one wave per instance.  The refusals are pdp_exact_count_round's
 * (PDP_ERR_INVALID naming the cube or instance, before anything is searched or written), with model rows past 2^31 bytes in place of its
 * rows of doubles.  R != 1 -> PDP_ERR_UNSUPPORTED.  Routing, slab and working arrays are pdp_exact_solve's.  The call synchronises the
 * stream once (the check's verdict). */
#define PDP_EXACT_SOLVE_ROUND_BUDGET (((int64_t)1) << 18)
int pdp_exact_solve_round(pdp_problem *p, const float *hint, const int64_t *cube_off, int64_t cubes, const int32_t *len,
                          const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status, float *model, int64_t *work,
                          int32_t *first, int8_t *cube_status, int32_t *len_out, uint32_t *bits_out, uint32_t *closed_out,
                          int64_t *cube_work, int64_t *cube_replay, void *stream);

/* pdp_exact_nearest as a sequence of rounds over the same frontier, with the bound exchanged between two rounds (plain Python, normative:
 * tests/exact_nearest_rounds_model.py).  The frontier (cube_off, len, bits, closed, the pairs,
 * pdp_exact_count_frontier_words), its check and the checkpoints are pdp_exact_count_round's, and the next frontier comes from
 * pdp_exact_count_expand, called as it is with this call's cube_status (it expands the cubes of status -1).
 *   Search of a cube.  pdp_exact_nearest's branch and bound without its check pass, with plen = len and ub = cost[b] as it stood when the
 *   round began (-1: infinite).  A decision that opens level L <= plen takes the hint's polarity for bit 0 and the other one for bit 1, and
 *   carries the flipped mark iff closed.  A bit-1 decision adds the variable's penalty to dist; if that reaches ub the state is pruned at
 *   once, before any pass.  A prune is pdp_exact_nearest's chronological backtracking (a flip whose penalty alone reaches ub is skipped
 *   and the level undone); it pops closed levels, and a flip of an open level L sets plen = min(plen, L).  A state without an open clause
 *   and dist < ub is accepted wherever it is met, also at a level < plen: ub = cube_cost = dist, one improvement, the cube's model = the
 *   assignment with the unassigned variables at their hint values; ub == 0 ends the cube, otherwise the state is pruned.  ub appears in
 *   the prune only -- the units are always forced and the branching variable does not read it -- so a path is replayed in the same tree
 *   under any bound: identically, or pruned earlier.  hint [V] may be NULL (all false), penalty [V] may be NULL (all 1).
 *   Budget of a round (reads per cube; budget <= 0: PDP_EXACT_NEAREST_ROUND_BUDGET) and checkpoint: pdp_exact_count_round's, word for
 *   word.  cube_status [cubes] = 1 (ended: nothing below the bound it ran under is left in it; len_out 0 and a row of zeros) or -1
 *   (stopped, with a checkpoint; it may have improved as well).  cube_cost [cubes] = the cube's last accepted cost, -1: none.
 *   Outcome, per instance that has a cube.  best = the minimum of the cube_cost >= 0.  If cost[b] < 0 or best < cost[b]: cost[b] = best,
 *   first[b] = the lowest cube, counted from cube_off[b], whose cube_cost is best, and model (its slice of [V]) = that cube's; else
 *   first[b] = -1 and cost and model stay.  work[b] and improvements[b] (in/out) take the integer sums over the cubes.  status[b] = 1 if
 *   cost[b] == 0, and the instance's stopped cubes get cube_status -2 ("dropped": the expansion leaves nothing of them, their checkpoints
 *   stay as written); else, if no cube stopped, 1 where cost[b] >= 0 and 0 where no model was ever met; else -1: cost is an upper bound
 *   that model attains, or -1.  An instance without a cube is not touched in any output.  cost, model, work and improvements are in/out:
 *   the caller starts them at -1, zeros (or a model it has checked and that model's distance), 0 and 0.  cube_cost, cube_work,
 *   cube_replay and cube_improvements [cubes] may be NULL.
 * No word is shared between two cubes inside a round and the only atomic is the counter that hands out cube ids, so every output, record
 * and frontier word is a function of the instances, hint, penalties, frontier, incoming cost and budget alone.  With one cube per
 * instance throughout (give 0) status, cost, model and the summed improvements are pdp_exact_nearest's bit for bit wherever that call's
 * check pass does not accept the hint, and the sum of cube_work - cube_replay over the rounds is its work less the check pass's reads;
 * where it accepts, the search follows the hint to cost 0 and model = the thresholded hint with one improvement.  With more cubes status
 * and cost are the same once the frontier is empty, and which minimiser comes back depends on budget and give.  One wave takes one cube at
 * a time; an accepted leaf leaves its assignment as a row of bytes in [cubes][n_max] on the handle; a last kernel writes the outcome, one
 * wave per instance.  The refusals are pdp_exact_solve_round's (PDP_ERR_INVALID naming the cube or instance, before anything is searched
 * or written), plus a penalty outside [0, 2^20] on an instance that has a cube.  R != 1 -> PDP_ERR_UNSUPPORTED.  Routing, slab and
 * working arrays are pdp_exact_solve's.  The call synchronises the stream once (the checks' verdicts). */
#define PDP_EXACT_NEAREST_ROUND_BUDGET (((int64_t)1) << 18)
int pdp_exact_nearest_round(pdp_problem *p, const float *hint, const int32_t *penalty, const int64_t *cube_off, int64_t cubes,
                            const int32_t *len, const uint32_t *bits, const uint32_t *closed, int64_t budget, int8_t *status, int64_t *cost,
                            float *model, int64_t *work, int32_t *improvements, int32_t *first, int8_t *cube_status, int32_t *len_out,
                            uint32_t *bits_out, uint32_t *closed_out, int64_t *cube_cost, int64_t *cube_work, int64_t *cube_replay,
                            int32_t *cube_improvements, void *stream);

/* The models of given ranks in pdp_exact_count's own order (plain Python, normative: tests/exact_rank_model.py).  The
 * counting search meets its leaves in a fixed depth-first order and a leaf with f unassigned variables stands for 2^f models, so "count
 * before the leaf + offset inside it" numbers every model of an instance exactly once.  Instance b asks for K_b = rank_off[b+1] -
 * rank_off[b] ranks, ranks[rank_off[b] ..), non-decreasing (duplicates allowed), each in 0 .. 2^53 - 1.  The search is pdp_exact_count's
 * -- passes, branching rule, backtracking, the budget check before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET), work < budget +
 * 3 * (edges of the instance), the leaf rule count = count + ldexp(1.0, n - trail length) -- without T, F, snap and the crediting, and
 * with a cursor over the instance's ranks:
 *   Leaf.  before = count, then the leaf rule.  While a rank is open and rank < count: o = rank - before in integers (both are below
 *      2^53: exact); an assigned variable takes its value, the j-th unassigned variable in ascending index (j from 0) takes bit j of o,
 *      bits from 53 up are 0; found = 1; the cursor moves on.  If no rank is open any more the search ends here, status 1, before any
 *      backtracking.  Emitting a model costs no work: work counts clause-literal reads only.
 *   End.  Out of levels: status 1, every open rank gets found = 0 ("there is no such model").  Budget: status -1, every open rank gets
 *      found = -1.  count_seen [B] = count at the end: the instance's model count if a rank >= that count was asked and status is 1,
 *      else the count up to and including the leaf of the last rank.
 *   Before any search.  More than 1023 variables: status -2, found = -1 for every rank, count_seen, work and leaves 0.  K_b = 0: status 1,
 *      count_seen 0.0, work and leaves 0.
 * found [rank_off[B]] (int8) and models (uint8, 0 / 1): instance b's rows start at byte sum over b' < b of K_b' * n_b', row j of them at
 * + j * n_b, one byte per variable of the instance (n counts every variable, also one in no clause); the row of a rank with found != 1 is
 * zero.  work and leaves [B] may be NULL; found and models may be NULL if rank_off[B] = 0.
 * Consequences: ranks 0 .. count - 1 enumerate the models of a complete count, each once; a call with a rank >= the instance's count has
 * pdp_exact_count's work, leaves and count, every other call at most those; the model of a rank is a function of the instance and the
 * rank alone -- it does not depend on the other ranks asked for, and under a smaller budget a rank is answered with the same model or
 * with found = -1.  count and before are uniform over the wave, one lane writes one byte of a row, and nothing goes through an atomic.
 * rank_off [B+1] and ranks are device int64.  PDP_ERR_INVALID, the message names the instance: rank_off[0] != 0, a decreasing rank_off,
 * a rank below 0 or >= 2^53, decreasing ranks inside an instance, more than 2^31 bytes of models (the instance at which the running
 * total passes the cap).  R != 1 -> PDP_ERR_UNSUPPORTED.  Routing, slab and working arrays are pdp_exact_solve's, shared with it.  The call
 * synchronises the stream once (it validates the ranks and sizes the rows); what follows is asynchronous on it. */
int pdp_exact_models_at(pdp_problem *p, const int64_t *rank_off, const int64_t *ranks, int64_t budget, int8_t *status, double *count_seen,
                        int8_t *found, uint8_t *models, int64_t *work, int64_t *leaves, void *stream);

/* pdp_exact_min_unsat with the search of every instance spread over 2^depth[b] waves that share one word, the best cost found so far
 * (plain Python, normative: tests/exact_min_unsat_split_model.py).  Same passes, same bound, same branching rule as
 * pdp_exact_min_unsat; same cubes as pdp_exact_solve_split: cube `index` of the 2^depth cubes of an instance is that search where the
 * decision of every level L <= depth is pinned -- the incumbent hint's polarity if bit (index >> (depth - L)) & 1 is 0, else the other
 * one -- and the level counts as already flipped, so backtracking pops through it and ends the cube.
 *   Check pass.  Once per instance, in a kernel of its own before the cubes; it always runs: the thresholded hint goes to model, its reads
 *      to chk, the clauses it leaves unsatisfied to ub0, and the shared word starts as ub[b] = ub0.  ub0 == 0: status 1, cost 0,
 *      first = -1, no cube is searched (cube status 1, work 0).
 *   Two bounds.  live is the cube's view of ub[b]: its own accepted cost at once, the other cubes' at the next re-read.  Every pass
 *      prunes on cost + contra >= live, at every level.  Case 2 of pdp_exact_min_unsat (all units are forced when cost == rule - 1) uses
 *      rule = ub0 while level < depth and rule = live once level >= depth.  The decisions of levels 1 .. depth are therefore taken in
 *      states that depend on the instance and its hint alone: all cubes agree on the prefix tree whatever the timing, and partition it.
 *      Forcing under ub0 is sound because live <= ub0; not forcing merely leaves a unit to a pinned decision.
 *   A prefix that ends early.  A prune while level < depth ends the cube (every open level is pinned).  A leaf met while level < depth
 *      belongs to the one cube with index & ((1 << (depth - level)) - 1) == 0; every other cube that reaches it ends there with nothing
 *      credited.
 *   Improvement.  A leaf (not pruned, no open clause) does one device-scope atomicMin(&ub[b], cost) and is accepted iff the old value
 *      was above cost.  On acceptance the cube writes its assignment (unassigned variables false) to its own row, records the cost as
 *      its cube_cost and one improvement more, and goes on with live = cost; otherwise live = the old value.  Either way it prunes.
 *   Budget.  Per cube: chk[b] + own reads >= budget before every pass (budget <= 0: PDP_EXACT_DEFAULT_BUDGET), so
 *      work < chk + cubes * (budget + 3 * edges of the instance).  At the same point the cube takes the minimum of live and the value of
 *      ub[b] it loaded at the previous check (a relaxed device-scope load by one lane, issued one pass ahead of its use; the first one
 *      before the cube copies the instance), ends as exhausted when live == 0, and only then tests the budget.  No wave waits for another.
 *   Finish (one wave per instance, sums in int64 and cube order).  cost = ub[b].  first [B] (int32, may be NULL) = the lowest cube whose
 *      cube_cost == cost, -1 if none: the thresholded hint stays in model; else model = that cube's row.  status 1 if every cube ended
 *      exhausted, else -1.  work = chk + the cubes' work.  improvements = the cubes' accepted improvements.
 * Promised.  At depth 0: pdp_exact_min_unsat's five outputs bit for bit under every budget.  At any depth with a budget that no cube
 * exhausts: status 1, cost = the minimum (pdp_exact_min_unsat's wherever that is proved), model leaves exactly cost clauses unsatisfied,
 * cube_cost[first] == cost, depth_used as requested (0 for an instance on the HBM route).  At any budget: cost is an upper bound that model
 * attains, cost <= ub0, and the work bound.  With one wave (PDP_EXACT_GRID=1) the cubes run in ascending order, each to its end, and every
 * output and record is the model's sequential().  NOT promised with more than one wave, because they depend on which cube lowers ub[b]
 * first: which minimiser model is, first, work, improvements, the cube records, and the status of a cube that ends near its budget.
 *   hint [V] (device; NULL: all false) as pdp_exact_min_unsat.  depth [B] (device int8; NULL: all 0) in 0 .. 16; at most 2^22 cubes per
 *   call; either violated -> PDP_ERR_INVALID, the message names the instance.  depth_used [B] (int8, may be NULL).  work, improvements
 *   and first may be NULL.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Routing and working arrays are pdp_exact_solve's, shared with it.  The call synchronises the stream once
 * (the cube count sizes its records and its grid); the kernels that follow are asynchronous on it. */
int pdp_exact_min_unsat_split(pdp_problem *p, const float *hint, const int8_t *depth, int64_t budget, int8_t *status, int32_t *cost,
                              float *model, int64_t *work, int32_t *improvements, int32_t *first, int8_t *depth_used, void *stream);

/* The per-cube records of the last pdp_exact_min_unsat_split call on the problem that succeeded (PDP_ERR_INVALID before the first and
 * after a refused one): cube_off [B+1] (int64), cube_status [cubes] (1 exhausted / -1 budget spent), cube_cost [cubes] (int32: the cube's
 * last accepted cost, -1: it accepted none), cube_work [cubes] (int64) and cube_improvements [cubes] (int32), cubes = cube_off[B] = the
 * sum of 2^depth_used.  Device to device, asynchronous on the stream. */
int pdp_exact_min_unsat_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int32_t *cube_cost, int64_t *cube_work,
                                    int32_t *cube_improvements, void *stream);

/* pdp_exact_nearest with the search of every instance spread over 2^depth[b] waves that share one 64-bit word, the cost of the best
 * model found so far (plain Python, normative: tests/exact_nearest_split_model.py).  Same passes, same bound, same
 * branching rule, penalties and thresholding as pdp_exact_nearest; same cubes as pdp_exact_solve_split: cube `index` of the 2^depth
 * cubes of an instance is that search where the decision of every level L <= depth is pinned -- the hint's polarity if bit
 * (index >> (depth - L)) & 1 is 0, else the other one -- and the level counts as already flipped, so backtracking pops through it and
 * ends the cube.  A pinned decision against the hint adds its penalty to dist at once; if dist >= live then, the cube ends before any pass.
 *   Check.  Once per instance, in a kernel of its own before the cubes.  A penalty outside [0, 2^20]: status -3, nothing is searched,
 *      every other output is 0 (start_cost -1).  Otherwise pdp_exact_nearest's check pass over the thresholded hint, its reads to chk:
 *      a model -> ub[b] = 0, status 1, cost 0, model = the hint, first = -1, no cube is searched (cube status 1, work 0); else ub[b] =
 *      infinity and model = 0.  With start != NULL it is thresholded like the hint and checked by one more such pass on every such
 *      instance, its reads added to chk: where it satisfies every clause, start_cost[b] = its penalty distance from the hint, computed
 *      by the kernel, and where that is below ub[b] it becomes ub[b] and the start model goes to model; where it does not, it is ignored
 *      and start_cost[b] = -1.  (A caller without a start model for some instance passes any assignment there.)
 *   One bound.  live is the cube's view of ub[b]: its own accepted cost at once, the other cubes' at the next re-read.  A conflict, a
 *      variable asked for twice or dist >= live prunes, at every level; a flip whose penalty brings dist to live is pruned before any
 *      pass.  The units are always forced and the branching variable does not depend on the bound, so all cubes agree on one prefix
 *      tree whatever the timing, and partition it.
 *   A prefix that ends early.  A prune while level < depth ends the cube.  A leaf met while level < depth belongs to the one cube with
 *      index & ((1 << (depth - level)) - 1) == 0; every other cube that reaches it ends there with nothing credited.
 *   Improvement.  A leaf (not pruned, no unit, no open clause) does one device-scope 64-bit atomic minimum on ub[b] with dist and is
 *      accepted iff the old value was above dist.  On acceptance the cube writes its assignment (an unassigned variable at its hint
 *      value) to its own row, records dist as its cube_cost and one improvement more, and goes on with live = dist; otherwise live =
 *      the old value.  Either way it prunes.
 *   Budget.  Per cube, before every pass, in this order: live = min(live, the value of ub[b] loaded at the previous check); live == 0
 *      ends the cube as exhausted; chk[b] + own reads >= budget ends it with status -1 (budget <= 0: PDP_EXACT_DEFAULT_BUDGET); one lane
 *      issues the next relaxed device-scope load.  The first load happens before the cube copies the instance.  So
 *      work < chk + cubes * (budget + 3 * edges of the instance).  No wave waits for another.
 *   Finish (one wave per instance, sums in int64 and cube order).  cost = ub[b], -1 while it is infinite.  first [B] (int32, may be
 *      NULL) = the lowest cube whose cube_cost == cost, -1 if none: model stays what the check wrote; else model = that cube's row.
 *      status -1 if any cube ran out of budget, else 1 if cost >= 0, else 0.  work = chk + the cubes' work.  improvements = the cubes'
 *      accepted ones.
 * Promised.  At depth 0 without a start model: pdp_exact_nearest's five outputs bit for bit under every budget.  At any depth with a
 * budget that no cube exhausts: status and cost are pdp_exact_nearest's, model satisfies every clause at penalty distance cost from the
 * hint, and cube_cost[first] == cost or first == -1 with cost 0 or start_cost; depth_used as requested (0 for an instance on the HBM
 * route).  At any budget: cost is -1 or an upper bound that model attains, cost <= start_cost where a start model was accepted, a
 * status -1 cost never rises with the budget, and the work bound.  With one wave (PDP_EXACT_GRID=1) the cubes run in ascending order,
 * each to its end, and every output and record is the model's sequential().  NOT promised with more than one wave, because they depend
 * on which cube lowers ub[b] first: which minimiser model is, first, work, improvements, the cube records, and the status of a cube
 * that ends near its budget.
 *   hint [V] (device; NULL: all false) and penalty [V] (device int32; NULL: all 1) as pdp_exact_nearest.  start [V] (device float; NULL:
 *   none).  depth [B] (device int8; NULL: all 0) in 0 .. 16; at most 2^22 cubes per call; either violated -> PDP_ERR_INVALID, the
 *   message names the instance, before any search is launched.  cost [B] int64.  work, improvements, first, depth_used [B] (int8) and
 *   start_cost [B] (int64) may be NULL.
 * R != 1 -> PDP_ERR_UNSUPPORTED.  Routing and working arrays are pdp_exact_solve's, shared with it.  The call synchronises the stream once
 * (the cube count sizes its records and its grid); the kernels that follow are asynchronous on it. */
int pdp_exact_nearest_split(pdp_problem *p, const float *hint, const int32_t *penalty, const float *start, const int8_t *depth,
                            int64_t budget, int8_t *status, int64_t *cost, float *model, int64_t *work, int32_t *improvements,
                            int32_t *first, int8_t *depth_used, int64_t *start_cost, void *stream);

/* The per-cube records of the last pdp_exact_nearest_split call on the problem that succeeded (PDP_ERR_INVALID before the first and
 * after a refused one): cube_off [B+1] (int64), cube_status [cubes] (1 exhausted / -1 budget spent), cube_cost [cubes] (int64: the cube's
 * last accepted cost, -1: it accepted none), cube_work [cubes] (int64) and cube_improvements [cubes] (int32), cubes = cube_off[B] = the
 * sum of 2^depth_used.  Device to device, asynchronous on the stream. */
int pdp_exact_nearest_split_cubes(pdp_problem *p, int64_t *cube_off, int8_t *cube_status, int64_t *cube_cost, int64_t *cube_work,
                                  int32_t *cube_improvements, void *stream);

/* *grid_host (a host int32) = the workgroups of the last launch that pdp_exact_solve, pdp_exact_solve_hinted, pdp_exact_solve_learn,
 * pdp_exact_solve_learn_proof, pdp_exact_solve_learn_assume, pdp_exact_min_unsat, pdp_exact_nearest, pdp_exact_count, pdp_exact_mass, pdp_exact_models_at, pdp_exact_solve_split, pdp_exact_count_split, pdp_exact_min_unsat_split, pdp_exact_nearest_split, pdp_exact_mass_split, pdp_exact_count_round, pdp_exact_solve_round and pdp_exact_nearest_round (their cube kernels:
 * min(cubes, CUs * resident workgroups per CU)), pdp_exact_check or pdp_exact_trim issued without an error on the problem; 0 before the first, and a call that fails
 * leaves the value.  Each of them launches min(B, CUs * resident workgroups per CU) workgroups of one wave that take instance after
 * instance from one counter; the environment variable PDP_EXACT_GRID=<v>, read at every launch, lowers that to min(grid, v) for an
 * integer v >= 1 and is ignored otherwise (unset, empty, 0, negative, not a number) -- a test switch that makes a wave run many
 * instances one after the other on a small batch; no output of the entry points above depends on the grid.  Reads a host field the
 * launches write: no synchronisation, no stream. */
int pdp_exact_last_grid(const pdp_problem *p, int32_t *grid_host);

/* ---- persistent solve: the whole _forward_core loop in one launch ------------------------------------
 * replaces: PropagatorDecimatorSolverBase._forward_core (solver.py:355-386) for the classical
 * triples (SurveyPropagator + SequentialDecimator + IdentityPredictor, or the Reinforce triple),
 * one workgroup per instance with the instance resident in LDS; instances past the LDS limit run
 * on an HBM-resident kernel inside the same call (per-instance routing; a big instance is spread
 * over a team of workgroups).  The kernels assume the reference's accidental cross-instance
 * couplings are inert (batch-global min == 0); a NaN survey, which poisons the whole batch in the
 * reference, is detected and the affected instances are replayed on the device.  If a coupling was
 * active the call restores every array it touched and reruns a batch of up to 1 024 instances in a
 * lock-step launch that exchanges the couplings exactly; a larger batch returns PDP_ERR_SPECULATION:
 * the caller reruns it through the step-wise entry points above.  A batch of ONE instance (or the
 * identical replicas of one) is solved exactly instead -- its batch-global minima are its own --
 * and never fails.  Synchronises. */
typedef struct pdp_solve_args {
    int32_t model;                /* PDP_MODEL_SP or PDP_MODEL_REINFORCE */
    int32_t iterations;           /* T */
    float tolerance, t_max, pi, decimation_probability;
    uint64_t seed;                /* reserved */
    const float *coins;           /* PDP_MODEL_REINFORCE: device array [iterations], the shared coin torch.rand(1) of every iteration
                                   * (pdp_decimate.py:218) drawn by the caller in order; iterations_run_host says how many were consumed */
    float *q;                     /* [E,3] in: init propagator state[0], out: final */
    float *fs;                    /* [E,2] in/out */
    uint8_t *active_mask;         /* [B] in/out */
    pdp_decimator *decimator;     /* in/out */
    int32_t check_termination;    /* 1: per-iteration CNF check de-activates solved instances */
    int32_t iterations_run_host;  /* out: executed iterations (max over instances) */
    int32_t used_lds_host;        /* out: 1 if the LDS-resident variant ran */
    int32_t kernel_launches_host; /* out: launches of the solver kernel that did work (one per chunk of iterations) */
    int32_t replay_launches_host; /* out: poison-replay launches that did work */
    int32_t time_kernels;         /* in: 1 = bracket every chunk launch with HIP events and report the sums below */
    float solve_kernel_ms_host;   /* out: device time of the chunk launches (time_kernels == 1) */
    float replay_kernel_ms_host;  /* out: device time from the end of a chunk launch that was replayed to the start of the next chunk's: the replay
                                   * launch and the four control kernels around it (time_kernels == 1) */
    int32_t replicas_identical;   /* in: 1 = the R replicas of every instance (batch replication, solver.py:56-82) start from identical state,
                                   * so their trajectories coincide and the replica-aware termination rule (trainer.py:157-160) equals the
                                   * per-replica one.  0 with replication > 1 (random initial state): the replicas couple through the
                                   * termination rule -- batches of up to 1 024 instances run in the lock-step launch, larger ones return
                                   * PDP_ERR_SPECULATION untouched */
    int32_t isolate_instances;    /* in: 1 = "fixed" semantics instead of the reference's: every instance is solved on its own -- the
                                   * batch-global minimum of sparse_max / sparse_argmax is taken as 0 and a NaN survey stops the decimation
                                   * of its own instance only (in the reference it stops the whole batch).  Never
                                   * returns PDP_ERR_SPECULATION. */
    int32_t hbm_instances_host;   /* out: instances of the batch that did not fit the LDS and ran on the HBM-resident kernel inside the same chunk
                                   * loop (per-instance routing; 0 when every instance fits, the batch size when none does) */
    int32_t inputs_disposable;    /* in: 1 = the caller does not need q / fs back when the call returns PDP_ERR_SPECULATION (it still holds the
                                   * state it built them from, as PropagatorDecimatorSolverBase does: its init_state is never mutated,
                                   * solver.py:355-365) -- the call then skips their call-entry snapshot (250 MB of copies on config 2).  Every
                                   * other array is restored as always; 0 keeps the full guarantee */
} pdp_solve_args;
int pdp_sp_solve(pdp_problem *p, pdp_solve_args *args, void *stream);

/* ---- DIMACS ingestion (host code, no GPU needed) -----------------------------------------------------------
 * Native twin of the reference's converter front end (reference: src/dimacs2json.py:22-51 parsing, :43-51,85-91
 * compaction; consumed by src/pdp/factorgraph/dataset.py:120-136).  pdp_dimacs_open parses one file in a single pass and
 * reports the sizes of the COMPACT instance (unused variables dropped, empty clauses dropped, last occurrence of a
 * variable inside a clause wins); pdp_dimacs_read copies the edge list: signed_vars[e] = +-(1-based compact variable id),
 * clause_ids[e] = 1-based clause id, clause-major with ascending variable index -- the second and third list of the
 * reference's JSON line.  Malformed input -> PDP_ERR_INVALID with file:line in pdp_last_error(). */
typedef struct pdp_dimacs pdp_dimacs;
int pdp_dimacs_open(const char *path, pdp_dimacs **out, int32_t *n_vars, int32_t *n_clauses, int64_t *n_edges);
int pdp_dimacs_read(const pdp_dimacs *d, int32_t *signed_vars /*[n_edges]*/, int32_t *clause_ids /*[n_edges]*/);
int pdp_dimacs_close(pdp_dimacs *d);
/* count files parsed by `threads` host threads; out / n_vars / n_clauses / n_edges are arrays of `count` entries.  On a failure every
 * handle is released and the first error is reported. */
int pdp_dimacs_open_many(const char *const *paths, int32_t count, int32_t threads, pdp_dimacs **out, int32_t *n_vars,
                         int32_t *n_clauses, int64_t *n_edges);

/* ---- neural plug-ins: per-edge MLP / GRU layers on the fp32 matrix cores ---------------------------------
 * Weights are handed over PRE-TRANSPOSED and ZERO PADDED by the host: a layer y = act(W x + b) with nn.Linear weight
 * W [N, K] is passed as Wt [Kp, Np] row-major with Wt[k, j] = W[j, k], Kp = K rounded up to even, Np = N rounded up
 * to a multiple of 32, biases padded to Np with zeros.  Products are k-ordered fp32 fma chains starting at the bias. */
typedef struct pdp_agg_desc {      /* MessageAggregator (reference: src/pdp/nn/util.py:11-77) */
    const float *Wt1m, *b1m, *Wt2m, *Wt1a, *b1a, *Wt2a;   /* W1_m (+bias), W2_m, W1_a (+bias), W2_a */
    int32_t din;                    /* input width = state width + 1 (edge sign is appended by the kernel) */
    int32_t m1, a, g, out;          /* mem_hidden, mem_agg_hidden, agg_hidden, output widths */
    int32_t fd;                     /* 1: edge sign appended after aggregation (include_self_message=False), else 0 */
} pdp_agg_desc;
typedef struct pdp_gru_desc {      /* nn.GRUCell: Wt_ih [Kp(dx+1), 3*Hp], Wt_hh [Kp(H), 3*Hp], gate g at columns g*Hp.. */
    const float *Wt_ih, *Wt_hh, *b_ih, *b_hh;
    int32_t dx, H;
} pdp_gru_desc;
typedef struct pdp_head_desc {     /* Perceptron / PerceptronTanh head: Wt1 [Kp(H), Np(C)], b1 [Np], w2 [C] */
    const float *Wt1, *b1, *w2;
    int32_t H, C, out_act;         /* out_act: 3 sigmoid (trainer.py:28-29), 4 tanh (util.py:250-251) */
} pdp_head_desc;
/* replaces: one MessageAggregator call of NeuralMessagePasser.forward (pdp_propagate.py:77-78 by_variable=1, :88-89
 * by_variable=0): out [E,out] = mask * Agg([state ‖ sign]) + (1 - mask) * old, mask from active_mask (NULL: ones) */
int pdp_neural_aggregate_edges(pdp_problem *p, const pdp_agg_desc *d, int by_variable, const float *state,
                               const float *edge_mask, const uint8_t *active_mask, const float *old, float *out, void *stream);
/* replaces: one GRU direction of NeuralDecimator.forward (pdp_decimate.py:70-75, 78-83): out [E,H] (must not alias h) */
int pdp_neural_gru(pdp_problem *p, const pdp_gru_desc *d, const float *state, const float *h, const uint8_t *active_mask,
                   float *out, void *stream);
/* replaces: NeuralPredictor.forward variable branch (pdp_predict.py:67-77): state [E,H] -> pred [V] */
int pdp_neural_predict(pdp_problem *p, const pdp_agg_desc *d, const pdp_head_desc *head, const float *state,
                       const float *edge_mask, float *pred, void *stream);

/* ---- training path (the gradients loss.backward() needs in FactorGraphTrainerBase._train_batch, src/pdp/factorgraph/base.py:149-182) ------------
 * The reference differentiates its torch operators with autograd.  Each differentiable building block of the np-nd-np solver has a
 * forward and an adjoint entry point here; the host wraps a pair in an autograd node (pdp/nn/train_ops.py) and keeps the graph bookkeeping,
 * gradient clipping and the caller's optimizer.  Activations are identified like pdp_head_desc.out_act: 0 none, 1 logsigmoid, 2 relu,
 * 3 sigmoid, 4 tanh; activation derivatives are taken from the saved OUTPUT.  All matrices row-major fp32. */
/* replaces: nn.Linear + activation (util.py:56,74 MessageAggregator layers; trainer.py:28-29 Perceptron): Y [R,N] = act(X [R,K] W^T + b), W [N,K] */
int pdp_train_linear(const float *X, int64_t R, int K, int64_t ldx, const float *W, const float *b, int N, int act, float *Y, void *stream);
/* adjoint: dZ = dY * act'(Y) (dZ [R,N]: scratch, may alias dY); dX [R,K] = dZ W (NULL: skipped); dW [N,K] = dZ^T X; db [N] = column sums (NULL: no bias) */
int pdp_train_linear_backward(const float *dY, const float *Y, const float *X, int64_t R, int K, int64_t ldx, const float *W, int N, int act,
                              float *dZ, float *dX, int64_t lddx, float *dW, float *db, void *stream);
/* The same layer on an operand whose LAST column is stored apart -- Y = act([X | xs] W^T + b) with X [R,K], xs [R] (the edge sign the reference
 * concatenates in front of every layer of the training path, pdp_propagate.py:66-67, util.py:71-72), W [N, K + 1]: the K-wide block runs on the
 * row-stripe GEMM, the last column is a rank-one term of its epilogue; no [R, K + 1] copy is made.  Only for shapes that kernel takes
 * (pdp_train_linear_s_supported != 0: >= 4 096 rows, act none / logsigmoid, the weight chunk fits the LDS); otherwise concatenate. */
int pdp_train_linear_s_supported(int64_t R, int K, int N, int act);
int pdp_train_linear_s(const float *X, const float *xs, int64_t R, int K, int64_t ldx, const float *W, const float *b, int N, int act, float *Y, void *stream);
/* adjoint: dX [R,K] = dZ W[:, :K] (NULL: skipped); dW [N, K + 1] = [ dZ^T X | dZ^T xs ]; db [N] (NULL: no bias); xs has no gradient */
int pdp_train_linear_s_backward(const float *dY, const float *Y, const float *X, const float *xs, int64_t R, int K, int64_t ldx, const float *W, int N, int act,
                                float *dZ, float *dX, int64_t lddx, float *dW, float *db, void *stream);
/* replaces: torch.mm(mask, state) of MessageAggregator.forward (util.py:60): x [E,A] -> out [rows,A], ordered sum over the edges of every
 * variable (by_variable != 0) or clause */
int pdp_train_row_sum(pdp_problem *p, int by_variable, const float *x, int A, float *out, void *stream);
/* replaces: torch.mm(mask_transpose, aggregated) - state (util.py:63-69): rows [rows,A] -> out [E,A] = rows[row(e)] - x[e] (x NULL: gather only).
 * The adjoint of the exclude-self aggregation is the same pair of calls on the gradient; of the plain row sum, the gather. */
int pdp_train_row_spread(pdp_problem *p, int by_variable, const float *rows, const float *x, int A, float *out, void *stream);
/* replaces: nn.GRUCell forward (pdp_decimate.py:38-41,70-83): x [R,Kx], h [R,H], W_ih [3H,Kx], W_hh [3H,H] -> hnew [R,H];
 * saved [R,4H] = r | z | n | W_hn h + b_hn for the adjoint; scratch [R,6H] */
int pdp_train_gru(const float *x, const float *h, const float *W_ih, const float *W_hh, const float *b_ih, const float *b_hh, int64_t R, int Kx, int H,
                  float *hnew, float *saved, float *scratch, void *stream);
/* the same forward for the hidden-128 cells of the shipped models (x = [state [R,dx] | sign [R]], dx = 128: np-nd-np, dx = 2 or 3: p-nd-np) in ONE
 * launch of the pipelined inference kernel, which also writes
 * saved [R,4H]: no gi / gh round trip through memory.  Weights in the descriptor layout of the inference cell -- transposed, padded; R a multiple of 64 (the caller runs
 * pdp_train_gru on the rows behind the last full tile). */
int pdp_train_gru_fused(const pdp_gru_desc *d, const float *state, const float *sign, const float *h, int64_t R, float *hnew, float *saved, void *stream);
/* adjoint: dhnew [R,H] -> dx [R,Kx], dh [R,H], dW_ih, dW_hh, db_ih [3H], db_hh [3H]; scratch [R,6H] (a [R,7H] block is fine) */
int pdp_train_gru_backward(const float *dhnew, const float *saved, const float *x, const float *h, const float *W_ih, const float *W_hh, int64_t R, int Kx,
                           int H, float *dx, float *dh, float *dW_ih, float *dW_hh, float *db_ih, float *db_hh, float *scratch, void *stream);
/* the adjoint for a cell whose input is [state [R,Ks] | xs [R]] held apart (W_ih [3H, Ks + 1]): dstate [R,Ks], dW_ih [3H, Ks + 1]; scratch [R,6H] */
int pdp_train_gru_backward_s(const float *dhnew, const float *saved, const float *state, const float *xs, const float *h, const float *W_ih, const float *W_hh,
                             int64_t R, int Ks, int H, float *dstate, float *dh, float *dW_ih, float *dW_hh, float *db_ih, float *db_hh, float *scratch, void *stream);
/* adjoint of pdp_sp_propagate_adapted (the adaptor form of SurveyPropagator.forward, pdp_propagate.py:163-221, as the training path runs it: no
 * active mask): upstream g_q [E,3] (surveys) and g_eta [E] (column 0 of the function state; the force column carries no gradient, torch.sign) ->
 * d_xlog [E] (gradient of the log-domain clause message = logsigmoid of the function projector's output) and d_eta_in [E] (gradient of
 * fs2[:,0] = sigmoid of the variable projector's first output).  xlog / fs2 / edge_mask as handed to the forward. */
int pdp_train_sp_adapted_backward(pdp_problem *p, const float *xlog, const float *fs2, const float *edge_mask, float pi, const float *g_q,
                                  const float *g_eta, float *d_xlog, float *d_eta_in, void *stream);
/* adjoint of pdp_sat_loss (SatLossEvaluator.forward, util.py:178-197) with respect to the prediction: dpred [V] = upstream * d loss / d pred */
int pdp_sat_loss_grad(pdp_problem *p, const float *pred, float coeff, float eps, int sharpness, float upstream, float *dpred, void *stream);

/* ---- the reference's L0 primitives in their original call shape (a sparse COO mask instead of a problem handle) ---------------------
 * For plug-ins written against the reference's API: they hand util.sparse_max / sparse_argmax /
 * sparse_smooth_max and MessageAggregator.forward the torch sparse masks of SATProblem (or masks they built themselves).  The host maps
 * the masks SATProblem built back to the resident layout (the entry points above); any other mask arrives here as its index / value
 * arrays.  No pdp_problem is involved.
 * replaces: util.sparse_max / sparse_argmax (util.py:257-275) for an arbitrary mask [n_rows, n_cols] given as nnz (row, col) pairs in
 * the order of mask._indices(); x [nnz] is paired with the entries in that order (the reference builds
 * sparse(mask._indices(), x - x.min() + 1).to_dense()); out [n_cols]; an empty column yields 0 (arg-max) / x.min() - 1 (max); NaN counts
 * as the largest value, ties go to the smallest row.  scratch: uint64 [n_cols + 2]. */
int pdp_coo_max(const int64_t *rows, const int64_t *cols, int64_t nnz, const float *x, int64_t n_rows, int64_t n_cols, uint64_t *scratch,
                float *out, void *stream);
int pdp_coo_argmax(const int64_t *rows, const int64_t *cols, int64_t nnz, const float *x, int64_t n_rows, int64_t n_cols, uint64_t *scratch,
                   int64_t *out, void *stream);
/* row offsets [n_rows + 1] of entries sorted by row (a coalesced torch sparse tensor) */
int pdp_coo_row_ptr(const int64_t *sorted_rows, int64_t nnz, int64_t n_rows, int64_t *row_ptr, void *stream);
/* replaces: torch.mm(mask, X) of util.py:60,63 for an arbitrary mask given as row offsets + columns (+ values, NULL: ones) of its row-sorted
 * entries: out [n_rows, d] = mask X [., d] (row stride ldx) - sub (NULL: nothing subtracted; the exclude-self form of util.py:63-69);
 * a row's entries are added in ascending entry order */
int pdp_csr_matmul(const int64_t *row_ptr, const int64_t *cols, const float *vals, int64_t n_rows, const float *X, int d, int64_t ldx,
                   const float *sub, float *out, void *stream);
/* replaces: util.sparse_smooth_max (util.py:282-286) for an arbitrary mask and alpha: x [n_cols] -> out [n_rows] */
int pdp_csr_smooth_max(const int64_t *row_ptr, const int64_t *cols, const float *vals, int64_t n_rows, const float *x, float alpha,
                       float *out, void *stream);

/* ---- kernel timing (measurement only: bench.py's per-kernel roofline lines) ------------------------------
 * When enabled, the library brackets the kernels named below with HIP events ON THEIR LAUNCH STREAM (the stream handed to the entry
 * point); pdp_kernel_timing_read synchronises on the recorded events and returns, per key, the summed device time in ms and the number
 * of launches since the last read.  No effect on results; off by default. */
enum { PDP_TK_AGG_PRE = 0,      /* k_agg_pre_wave / k_agg_pre_res / k_agg_pre: first half of a MessageAggregator (two layers per edge) */
       PDP_TK_ROW_SUM = 1,      /* k_row_sum: per-row sum of the pre-transformed edges */
       PDP_TK_AGG_POST = 2,     /* k_agg_post_pf / k_agg_post_wave (hidden 150) / k_agg_post: second half (two layers per edge, masked blend) */
       PDP_TK_GRU = 3,          /* k_gru_pipe (hidden 128) / k_gru_wave (hidden 150) / k_gru */
       PDP_TK_PREDICT_HEAD = 4, /* k_predict_rows: per-variable layers + perceptron head of NeuralPredictor */
       PDP_TK_WALKSAT = 5,      /* k_walksat<uint16_t, 256>: the persistent LDS-resident Walk-SAT launch of pdp_local_search */
       PDP_TK_SP_ADAPTORS = 6,  /* k_sp_adaptors: the two projections in front of the adaptor form of the SP sweep (p-nd-np) */
       PDP_TK_SP_SWEEP = 7,     /* k_sp_propagate<false|true>: the step-wise SP sweep (pdp_sp_propagate / pdp_sp_propagate_adapted) */
       PDP_TK_COUNT = 8,
       /* name-only keys (their times come back through pdp_solve_args) */
       PDP_KN_SP_SOLVE = 8,     /* pass 1 of pdp_sp_solve (k_sp_solve_lds<...> / k_sp_solve<...>) */
       PDP_KN_SP_REPLAY = 9,    /* its NaN-poison replay instantiation */
       PDP_KN_COUNT = 10 };
int pdp_kernel_timing(int enable);
/* the name (with template arguments, as rocprofv3 prints it) of the kernel the library launched last for `key`; empty before the first launch */
int pdp_kernel_name(int key, char *buf, int len);
int pdp_kernel_timing_read(float *ms_host /*[PDP_TK_COUNT]*/, int32_t *launches_host /*[PDP_TK_COUNT]*/);

/* ---- math probes (tests: device exp/log must equal the host header bit for bit) ---------------------- */
int pdp_math_apply(int fn, const float *x, float *y, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDP_HIP_H */
