"""ctypes binding of libpdp_hip.so (the C ABI declared in include/pdp_hip.h).

PyTorch is used for device memory and streams only: every call hands raw device pointers
(``tensor.data_ptr()``) and the current HIP stream to the library.  There is NO CPU fallback: if the
library is missing or no GPU is visible the calls raise (loudly), they never reroute.
"""

import ctypes as C
import numbers
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# two builds of the same sources (csrc/Makefile): 'parity' -- the default, IEEE-only device math, the oracle's bits -- and the opt-in 'fast'
# (device math on the transcendental unit, include/pdp_math.h PDP_FAST_MATH; gated by the reference-held fixtures only).  PDP_BUILD=fast
# selects it for a process, use_build() inside one; PDP_HIP_LIB names any other file (A/B builds).
BUILDS = {'parity': 'libpdp_hip.so', 'fast': 'libpdp_hip_fast.so'}
BUILD = os.environ.get('PDP_BUILD', 'parity')
if BUILD not in BUILDS:
    raise ImportError("PDP_BUILD must be one of %s, got %r" % (sorted(BUILDS), BUILD))
LIB_PATH = os.environ.get('PDP_HIP_LIB') or os.path.join(os.path.dirname(_HERE), 'csrc', BUILDS[BUILD])

PDP_OK = 0
PROOF_WORDS_PER_LITERAL = 8      # default proof region of an instance (Problem.exact_solve_proof), in words per literal: the smallest power of two that truncates no proof of tools/exact_time.py pa pm100 pm200; too few costs a retry, never an answer
PDP_ERR_SPECULATION = 5
RNG_STREAM, RNG_PHILOX = 0, 1
MODEL_SP, MODEL_WALKSAT, MODEL_REINFORCE = 0, 1, 2

EXPORTED_SYMBOLS = [
    'pdp_abi_version', 'pdp_last_error', 'pdp_device_count', 'pdp_problem_create', 'pdp_problem_destroy',
    'pdp_problem_dims', 'pdp_problem_set_rng_base', 'pdp_problem_set_exchange', 'pdp_problem_export_graph', 'pdp_problem_bind_state', 'pdp_simplify', 'pdp_set_variables',
    'pdp_refresh_edge_mask', 'pdp_smooth_max', 'pdp_instance_max', 'pdp_instance_argmax', 'pdp_sp_propagate', 'pdp_sp_adaptors', 'pdp_sp_propagate_adapted',
    'pdp_survey_score', 'pdp_cnf_eval', 'pdp_sat_loss', 'pdp_update_solution', 'pdp_check_termination', 'pdp_loop_begin', 'pdp_loop_step', 'pdp_loop_read', 'pdp_decimator_create',
    'pdp_decimator_destroy', 'pdp_decimator_reset', 'pdp_sequential_decimate', 'pdp_sequential_decimate_gate',
    'pdp_sequential_decimate_apply', 'pdp_reinforce_decimate', 'pdp_reinforce_predict', 'pdp_energy',
    'pdp_energy_diff', 'pdp_random_fill', 'pdp_local_search', 'pdp_deduplicate', 'pdp_sp_solve', 'pdp_math_apply',
    'pdp_neural_aggregate_edges', 'pdp_neural_gru', 'pdp_neural_predict', 'pdp_dimacs_open', 'pdp_dimacs_read', 'pdp_dimacs_close', 'pdp_dimacs_open_many',
    'pdp_kernel_timing', 'pdp_kernel_timing_read', 'pdp_kernel_name',
    'pdp_train_linear', 'pdp_train_linear_backward', 'pdp_train_linear_s_supported', 'pdp_train_linear_s', 'pdp_train_linear_s_backward', 'pdp_train_row_sum', 'pdp_train_row_spread', 'pdp_train_gru', 'pdp_train_gru_fused', 'pdp_train_gru_backward', 'pdp_train_gru_backward_s',
    'pdp_sat_loss_grad', 'pdp_train_sp_adapted_backward',
    'pdp_coo_max', 'pdp_coo_argmax', 'pdp_coo_row_ptr', 'pdp_csr_matmul', 'pdp_csr_smooth_max',
    'pdp_exact_solve', 'pdp_exact_solve_hinted', 'pdp_exact_solve_learn', 'pdp_exact_learn_reductions',
    'pdp_exact_solve_learn_proof', 'pdp_exact_check', 'pdp_exact_trim', 'pdp_exact_last_grid', 'pdp_exact_solve_learn_assume',
    'pdp_exact_min_unsat', 'pdp_exact_count', 'pdp_exact_solve_split', 'pdp_exact_split_cubes',
    'pdp_exact_count_split', 'pdp_exact_count_split_cubes', 'pdp_exact_models_at',
    'pdp_exact_min_unsat_split', 'pdp_exact_min_unsat_split_cubes', 'pdp_exact_mass',
    'pdp_exact_mass_split', 'pdp_exact_mass_split_cubes', 'pdp_exact_nearest',
    'pdp_exact_nearest_split', 'pdp_exact_nearest_split_cubes',
    'pdp_exact_count_frontier_words', 'pdp_exact_count_round', 'pdp_exact_count_expand', 'pdp_exact_solve_round',
    'pdp_exact_nearest_round',
]


class NativeError(RuntimeError):
    pass


class SpeculationFailed(NativeError):
    """The persistent solver met one of the reference's cross-instance couplings; rerun step-wise."""


class CoupledForwardFailed(NativeError):
    """A coupled forward spread over several processes (--split-forward) met a coupling only the single-process loops reproduce (the
    batch-global minimum of a sweep was not 0 in any part).  Every part raises it (the outcome is agreed on across the parts); the predict
    driver then solves that segment whole on the rank of its first part."""


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError("libpdp_hip.so is not built (%s); run `make -C pdp-solver_amd/csrc` or "
                              "__graft_entry__.build()" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.pdp_last_error.restype = C.c_char_p
        for name in EXPORTED_SYMBOLS:
            if name != 'pdp_last_error':
                getattr(_lib, name).restype = C.c_int
    return _lib


def use_build(name):
    """Switch this process to the other build of the library.  Handles (Problem, Decimator, weight descriptors) belong to the library that
    made them: drop every one of them first.  Returns the previous build's name."""
    global _lib, LIB_PATH, BUILD
    if name not in BUILDS:
        raise NativeError("unknown build %r (have %s)" % (name, sorted(BUILDS)))
    previous = BUILD
    if name != BUILD:
        BUILD = name
        LIB_PATH = os.path.join(os.path.dirname(_HERE), 'csrc', BUILDS[name])
        _lib = None
    return previous


def check(status):
    if status == PDP_OK:
        return
    msg = lib().pdp_last_error().decode('utf-8', 'replace')
    if status == PDP_ERR_SPECULATION:
        raise SpeculationFailed(msg)
    raise NativeError("libpdp_hip error %d: %s" % (status, msg))


def require_gpu():
    if not torch.cuda.is_available():
        raise NativeError("no HIP device visible: the PDP hot path has no CPU fallback")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_DT = {torch.float32: 'f32', torch.int32: 'i32', torch.uint8: 'u8', torch.int64: 'i64'}


def ptr(t, dtype=None, numel=None, name='tensor'):
    """Device pointer of a dense tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise NativeError("%s must live on the GPU" % name)
    if not t.is_contiguous():
        raise NativeError("%s must be contiguous" % name)
    if dtype is not None and t.dtype != dtype:
        raise NativeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if numel is not None and t.numel() != numel:
        raise NativeError("%s must have %d elements, got %d" % (name, numel, t.numel()))
    return C.c_void_p(t.data_ptr())


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32), C.c_int)


class SolveArgs(C.Structure):
    _fields_ = [('model', C.c_int32), ('iterations', C.c_int32), ('tolerance', C.c_float), ('t_max', C.c_float),
                ('pi', C.c_float), ('decimation_probability', C.c_float), ('seed', C.c_uint64),
                ('coins', C.c_void_p), ('q', C.c_void_p), ('fs', C.c_void_p), ('active_mask', C.c_void_p),
                ('decimator', C.c_void_p), ('check_termination', C.c_int32), ('iterations_run_host', C.c_int32),
                ('used_lds_host', C.c_int32), ('kernel_launches_host', C.c_int32), ('replay_launches_host', C.c_int32),
                ('time_kernels', C.c_int32), ('solve_kernel_ms_host', C.c_float), ('replay_kernel_ms_host', C.c_float),
                ('replicas_identical', C.c_int32), ('isolate_instances', C.c_int32), ('hbm_instances_host', C.c_int32),
                ('inputs_disposable', C.c_int32)]


class AggDesc(C.Structure):
    _fields_ = [('Wt1m', C.c_void_p), ('b1m', C.c_void_p), ('Wt2m', C.c_void_p), ('Wt1a', C.c_void_p), ('b1a', C.c_void_p),
                ('Wt2a', C.c_void_p), ('din', C.c_int32), ('m1', C.c_int32), ('a', C.c_int32), ('g', C.c_int32),
                ('out', C.c_int32), ('fd', C.c_int32)]


class GruDesc(C.Structure):
    _fields_ = [('Wt_ih', C.c_void_p), ('Wt_hh', C.c_void_p), ('b_ih', C.c_void_p), ('b_hh', C.c_void_p), ('dx', C.c_int32), ('H', C.c_int32)]


class HeadDesc(C.Structure):
    _fields_ = [('Wt1', C.c_void_p), ('b1', C.c_void_p), ('w2', C.c_void_p), ('H', C.c_int32), ('C', C.c_int32), ('out_act', C.c_int32)]


def _pad_linear(weight, bias):
    "nn.Linear weight [N,K] (+bias) -> (Wt [Kp,Np] zero padded, bias [Np]) in the layout include/pdp_hip.h documents"
    N, K = weight.shape
    Kp, Np = K + (K & 1), (N + 31) // 32 * 32
    Wt = torch.zeros(Kp, Np, dtype=torch.float32, device=weight.device)
    Wt[:K, :N] = weight.detach().t()
    bp = torch.zeros(Np, dtype=torch.float32, device=weight.device)
    if bias is not None:
        bp[:N] = bias.detach()
    return Wt.contiguous(), bp


class AggregatorWeights(object):
    "device-side, padded copy of a MessageAggregator's four layers (keeps the tensors alive for the descriptor)"

    def __init__(self, W1m, b1m, W2m, W1a, b1a, W2a, feature_dim):
        self.t = []
        Wt1m, bb1m = _pad_linear(W1m, b1m); Wt2m, _ = _pad_linear(W2m, None)
        Wt1a, bb1a = _pad_linear(W1a, b1a); Wt2a, _ = _pad_linear(W2a, None)
        self.t = [Wt1m, bb1m, Wt2m, Wt1a, bb1a, Wt2a]
        d = AggDesc()
        d.Wt1m, d.b1m, d.Wt2m, d.Wt1a, d.b1a, d.Wt2a = [x.data_ptr() for x in self.t]
        d.din = W1m.shape[1]; d.m1 = W1m.shape[0]; d.a = W2m.shape[0]; d.g = W1a.shape[0]; d.out = W2a.shape[0]; d.fd = feature_dim
        assert W1a.shape[1] == d.a + feature_dim
        self.desc = d


class GruWeights(object):
    def __init__(self, W_ih, W_hh, b_ih, b_hh):
        H = W_hh.shape[1]; dx1 = W_ih.shape[1]
        Hp = (H + 31) // 32 * 32
        Kpx, Kph = dx1 + (dx1 & 1), H + (H & 1)
        dev = W_ih.device
        Wt_ih = torch.zeros(Kpx, 3 * Hp, dtype=torch.float32, device=dev); Wt_hh = torch.zeros(Kph, 3 * Hp, dtype=torch.float32, device=dev)
        bi = torch.zeros(3 * Hp, dtype=torch.float32, device=dev); bh = torch.zeros(3 * Hp, dtype=torch.float32, device=dev)
        for g in range(3):
            Wt_ih[:dx1, g * Hp:g * Hp + H] = W_ih.detach()[g * H:(g + 1) * H].t()
            Wt_hh[:H, g * Hp:g * Hp + H] = W_hh.detach()[g * H:(g + 1) * H].t()
            bi[g * Hp:g * Hp + H] = b_ih.detach()[g * H:(g + 1) * H]; bh[g * Hp:g * Hp + H] = b_hh.detach()[g * H:(g + 1) * H]
        self.t = [Wt_ih.contiguous(), Wt_hh.contiguous(), bi, bh]
        d = GruDesc()
        d.Wt_ih, d.Wt_hh, d.b_ih, d.b_hh = [x.data_ptr() for x in self.t]
        d.dx = dx1 - 1; d.H = H
        self.desc = d


class HeadWeights(object):
    def __init__(self, W1, b1, W2, out_act):
        Wt1, bb1 = _pad_linear(W1, b1)
        w2 = W2.detach().reshape(-1).to(torch.float32).contiguous()
        self.t = [Wt1, bb1, w2]
        d = HeadDesc()
        d.Wt1, d.b1, d.w2 = [x.data_ptr() for x in self.t]
        d.H = W1.shape[1]; d.C = W1.shape[0]; d.out_act = {'sigmoid': 3, 'tanh': 4}[out_act]
        self.desc = d


class Decimator(object):
    """Native SequentialDecimator / ReinforceDecimator state (previous survey + counters)."""

    def __init__(self, problem):
        self.problem = problem
        h = C.c_void_p()
        self._made_by = lib()                         # a handle is destroyed by the library that made it, whatever build the process uses by then
        check(self._made_by.pdp_decimator_create(C.byref(h), problem._h))
        self._h = h

    def reset(self):
        check(lib().pdp_decimator_reset(self._h, _stream()))

    def __del__(self):
        try:
            if self._h:
                self._made_by.pdp_decimator_destroy(self._h)
                self._h = None
        except Exception:
            pass


COUNT_ROUNDS_MAX_N = 1023           # pdp_exact_count_round searches instances of up to this many variables, as pdp_exact_count
COUNT_ROUNDS_MAX_CUBES = 1 << 22    # cubes of one frontier
EXACT_NEAREST_MAX_PENALTY = 1 << 20 # pdp_exact_nearest and pdp_exact_nearest_round: a penalty is an integer in [0, 2^20]


class _RoundState(object):
    """What the three resumable states share: plain tensors named by FIELDS, KINDS[field] = (dtype, shape kind), the shape kinds being
    'B', 'V', 'B+1', 'cubes' and 'cubes x words'."""
    FIELDS = ()
    KINDS = {}
    FRONTIER = {'cube_off': (torch.int64, 'B+1'), 'len': (torch.int32, 'cubes'), 'bits': (torch.int32, 'cubes x words'),
                'closed': (torch.int32, 'cubes x words')}

    @property
    def cubes(self):
        return int(self.len.numel())

    def to(self, device):
        "a copy on ``device``"
        s = type(self)()
        for f in self.FIELDS:
            setattr(s, f, getattr(self, f).to(device).clone())
        return s

    def cpu(self):
        return self.to('cpu')

    def validate(self, problem):
        "what the library cannot see from raw pointers: devices, dtypes and shapes (the frontier's contents are checked on the GPU)"
        cubes = int(self.len.numel())
        words = C.c_int32()
        check(lib().pdp_exact_count_frontier_words(problem._h, C.byref(words)))
        shapes = {'B': (problem.B,), 'V': (problem.V,), 'B+1': (problem.B + 1,), 'cubes': (cubes,), 'cubes x words': (cubes, words.value)}
        for f in self.FIELDS:
            t = getattr(self, f)
            kind, size = self.KINDS[f][0], shapes[self.KINDS[f][1]]
            if not torch.is_tensor(t) or t.device != problem.device or t.dtype != kind or tuple(t.shape) != size or not t.is_contiguous():
                raise NativeError("state.%s must be a contiguous %s tensor of shape %s on %s" % (f, kind, size, problem.device))
        if cubes > COUNT_ROUNDS_MAX_CUBES:
            raise NativeError("state holds %d cubes; a frontier holds at most 2^22" % cubes)


class CountState(_RoundState):
    """A resumable count (Problem.exact_count_begin / exact_count_round): plain tensors, so it can be saved, moved with cpu() / to() and
    continued on another Problem built from the same items.  The frontier: cube_off int64 [B+1], len int32 [cubes], bits and closed int32
    [cubes, words] (two bits per decision level, include/pdp_hip.h).  The running totals: count float64 [B], true_count float64 [V],
    work and leaves int64 [B].  status int8 [B]: 1 complete, -1 cubes are open (count is a lower bound), -2 not searched; rounds int32
    [B]: the rounds the instance had a cube in."""
    FIELDS = ('cube_off', 'len', 'bits', 'closed', 'count', 'true_count', 'work', 'leaves', 'status', 'rounds')
    KINDS = dict(_RoundState.FRONTIER, count=(torch.float64, 'B'), true_count=(torch.float64, 'V'), work=(torch.int64, 'B'),
                 leaves=(torch.int64, 'B'), status=(torch.int8, 'B'), rounds=(torch.int32, 'B'))


class SolveState(_RoundState):
    """A resumable deciding search (Problem.exact_solve_begin / exact_solve_round): plain tensors, so it can be saved, moved with cpu() /
    to() and continued on another Problem built from the same items.  The frontier is CountState's: cube_off int64 [B+1], len int32
    [cubes], bits and closed int32 [cubes, words].  hint float32 [V]: the phase hints of every round (NaN: none).  status int8 [B]: -1
    cubes are open, 1 satisfiable, 0 unsatisfiable, -2 not searched (more than 1023 variables); model float32 [V]: the model of an
    instance of status 1, zeros elsewhere; work int64 [B]: the reads of all its cubes and rounds; rounds int32 [B]: the rounds the
    instance had a cube in."""
    FIELDS = ('cube_off', 'len', 'bits', 'closed', 'hint', 'status', 'model', 'work', 'rounds')
    KINDS = dict(_RoundState.FRONTIER, hint=(torch.float32, 'V'), status=(torch.int8, 'B'), model=(torch.float32, 'V'),
                 work=(torch.int64, 'B'), rounds=(torch.int32, 'B'))


class NearestState(_RoundState):
    """A resumable nearest-model search (Problem.exact_nearest_begin / exact_nearest_round): plain tensors, so it can be saved, moved with
    cpu() / to() and continued on another Problem built from the same items.  The frontier is CountState's: cube_off int64 [B+1], len
    int32 [cubes], bits and closed int32 [cubes, words].  hint float32 [V]: the point the distance is measured from (> 0.5 true, every
    other value false); penalty int32 [V]: what a variable costs where it differs.  status int8 [B]: -1 cubes are open, 1 cost is the
    minimum (or 0 was reached), 0 the instance has no model, -2 not searched (more than 1023 variables), -3 a penalty outside [0, 2^20];
    cost int64 [B]: the distance of model, an upper bound while the status is -1, -1: no model yet; model float32 [V]; work int64 [B]:
    the reads of all its cubes and rounds; improvements int32 [B]: the leaves its cubes accepted; rounds int32 [B]: the rounds the
    instance had a cube in."""
    FIELDS = ('cube_off', 'len', 'bits', 'closed', 'hint', 'penalty', 'status', 'cost', 'model', 'work', 'improvements', 'rounds')
    KINDS = dict(_RoundState.FRONTIER, hint=(torch.float32, 'V'), penalty=(torch.int32, 'V'), status=(torch.int8, 'B'),
                 cost=(torch.int64, 'B'), model=(torch.float32, 'V'), work=(torch.int64, 'B'), improvements=(torch.int32, 'B'),
                 rounds=(torch.int32, 'B'))


class Problem(object):
    """HBM-resident batch of CNF instances (native SATProblem)."""

    def __init__(self, graph_map, batch_variable_map, batch_function_map, edge_feature, batch_size=None, replication=1):
        require_gpu()
        L = lib()
        self.device = graph_map.device
        gm = graph_map.to(torch.int32).contiguous()
        bvm = batch_variable_map.to(torch.int32).contiguous()
        bfm = batch_function_map.to(torch.int32).contiguous()
        ef = edge_feature.to(torch.float32).reshape(-1).contiguous()
        E, V, F = gm.size(1), bvm.numel(), bfm.numel()
        if batch_size is None:
            batch_size = int(bvm.max().item()) + 1
        h = C.c_void_p()
        check(L.pdp_problem_create(C.byref(h), C.c_int(E), C.c_int(V), C.c_int(F), C.c_int(batch_size), C.c_int(replication),
                                   ptr(gm, torch.int32), ptr(bvm, torch.int32), ptr(bfm, torch.int32), ptr(ef, torch.float32),
                                   _stream()))
        self._h = h
        self._made_by = L                             # destroyed by the library that made it (see Decimator)
        dims = (C.c_int32 * 8)()
        check(L.pdp_problem_dims(self._h, dims))
        self.E, self.V, self.F, self.B, self.R, self.max_n, self.max_m, self.max_e = [int(x) for x in dims]
        dev = self.device
        self.active_variables = torch.empty(self.V, 1, dtype=torch.float32, device=dev)
        self.active_functions = torch.empty(self.F, 1, dtype=torch.float32, device=dev)
        self.solution = torch.empty(self.V, dtype=torch.float32, device=dev)
        self.is_sat = torch.empty(self.B, dtype=torch.float32, device=dev)
        self.edge_mask = torch.empty(self.E, 1, dtype=torch.float32, device=dev)
        check(L.pdp_problem_bind_state(self._h, ptr(self.active_variables), ptr(self.active_functions), ptr(self.solution),
                                       ptr(self.is_sat), ptr(self.edge_mask), _stream()))

    def __del__(self):
        try:
            if self._h:
                self._made_by.pdp_problem_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- graph export (replicated arrays for the python-visible attributes) --------------------------------
    def export_graph(self):
        dev = self.device
        gm = torch.empty(2, self.E, dtype=torch.int32, device=dev)
        bvm = torch.empty(self.V, dtype=torch.int32, device=dev)
        bfm = torch.empty(self.F, dtype=torch.int32, device=dev)
        ef = torch.empty(self.E, 1, dtype=torch.float32, device=dev)
        check(lib().pdp_problem_export_graph(self._h, ptr(gm), ptr(bvm), ptr(bfm), ptr(ef), _stream()))
        return gm, bvm, bfm, ef

    # -- K7 / K8 ---------------------------------------------------------------------------------------------
    def simplify(self):
        check(lib().pdp_simplify(self._h, _stream()))

    def set_variables(self, assignment):
        check(lib().pdp_set_variables(self._h, ptr(assignment, torch.float32, self.V, 'assignment'), _stream()))

    def refresh_edge_mask(self, want_flag=True):
        flag = C.c_int32(0)
        check(lib().pdp_refresh_edge_mask(self._h, C.byref(flag) if want_flag else None, _stream()))
        return bool(flag.value) if want_flag else None

    # -- K4 / K5 ---------------------------------------------------------------------------------------------
    def smooth_max(self, x):
        out = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_smooth_max(self._h, ptr(x, torch.float32, self.E, 'x'), ptr(out), _stream()))
        return out

    def instance_max(self, x):
        out = torch.empty(self.B, dtype=torch.float32, device=self.device)
        check(lib().pdp_instance_max(self._h, ptr(x, torch.float32, self.V, 'x'), ptr(out), _stream()))
        return out

    def instance_argmax(self, x):
        out = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_instance_argmax(self._h, ptr(x, torch.float32, self.V, 'x'), ptr(out), _stream()))
        return out

    # -- K1-K3, K6 -------------------------------------------------------------------------------------------
    def sp_propagate(self, dec_q, dec_fs, edge_mask, active_mask, init_q, init_fs, pi=0.0):
        out_q = torch.empty(self.E, 3, dtype=torch.float32, device=self.device)
        out_fs = torch.empty(self.E, 2, dtype=torch.float32, device=self.device)
        check(lib().pdp_sp_propagate(self._h, ptr(dec_q, torch.float32, 3 * self.E, 'decimator_state[0]'),
                                     ptr(dec_fs, torch.float32, 2 * self.E, 'decimator_state[1]'),
                                     ptr(edge_mask, torch.float32, self.E, 'edge_mask'),
                                     ptr(active_mask, torch.uint8, self.B, 'active_mask'),
                                     ptr(init_q, torch.float32, 3 * self.E, 'init_state[0]'),
                                     ptr(init_fs, torch.float32, 2 * self.E, 'init_state[1]'),
                                     C.c_float(pi), ptr(out_q), ptr(out_fs), _stream()))
        return out_q, out_fs

    def sp_adaptors(self, dec_v, dec_f, w_f, W_v):
        "adaptor form of the propagator inputs (p-nd-np): [E,H] decimator states -> xlog [E], fs2 [E,2]"
        H = dec_v.shape[1]
        xlog = torch.empty(self.E, dtype=torch.float32, device=self.device)
        fs2 = torch.empty(self.E, 2, dtype=torch.float32, device=self.device)
        check(lib().pdp_sp_adaptors(self._h, C.c_int(H), ptr(dec_v, torch.float32, self.E * H, 'decimator_state[0]'),
                                    ptr(dec_f, torch.float32, self.E * H, 'decimator_state[1]'), ptr(w_f, torch.float32, H, 'w_f'),
                                    ptr(W_v, torch.float32, 2 * H, 'W_v'), ptr(xlog), ptr(fs2), _stream()))
        return xlog, fs2

    def sp_propagate_adapted(self, xlog, dec_fs, edge_mask, active_mask, init_q, init_fs, pi=0.0, out=None):
        out_q = torch.empty(self.E, 3, dtype=torch.float32, device=self.device) if out is None else out[0]
        out_fs = torch.empty(self.E, 2, dtype=torch.float32, device=self.device) if out is None else out[1]
        check(lib().pdp_sp_propagate_adapted(self._h, ptr(xlog, torch.float32, self.E, 'xlog'), ptr(dec_fs, torch.float32, 2 * self.E, 'fs2'),
                                             ptr(edge_mask, torch.float32, self.E, 'edge_mask'), ptr(active_mask, torch.uint8, self.B, 'active_mask'),
                                             ptr(init_q, torch.float32, 3 * self.E, 'init_state[0]'), ptr(init_fs, torch.float32, 2 * self.E, 'init_state[1]'),
                                             C.c_float(pi), ptr(out_q, torch.float32, 3 * self.E, 'out[0]'), ptr(out_fs, torch.float32, 2 * self.E, 'out[1]'), _stream()))
        return out_q, out_fs

    def survey_score(self, fs, pi=0.0):
        out = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_survey_score(self._h, ptr(fs, torch.float32, 2 * self.E, 'message_state[1]'), C.c_float(pi), ptr(out), _stream()))
        return out

    # -- K9 / K13 --------------------------------------------------------------------------------------------
    def cnf_eval(self, pred):
        solved = torch.empty(self.B, 1, dtype=torch.float32, device=self.device)
        unsat = torch.empty(self.B, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_cnf_eval(self._h, ptr(pred, torch.float32, self.V, 'prediction'), ptr(solved), ptr(unsat), _stream()))
        return solved, unsat

    def sat_loss(self, pred, coeff, eps, sharpness):
        "energy loss of a prediction (SatLossEvaluator.forward): device float [1]"
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        check(lib().pdp_sat_loss(self._h, ptr(pred, torch.float32, self.V, 'prediction'), C.c_float(coeff), C.c_float(eps),
                                 C.c_int(int(sharpness)), ptr(out), _stream()))
        return out

    def update_solution(self, pred):
        out = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_update_solution(self._h, ptr(pred, torch.float32, self.V, 'prediction'), ptr(out), _stream()))
        return out

    def check_termination(self, active_mask, pred):
        check(lib().pdp_check_termination(self._h, ptr(active_mask, torch.uint8, self.B, 'active_mask'),
                                          ptr(pred, torch.float32, self.V, 'prediction'), _stream()))

    # -- device-driven loop (pdp_loop_*): the sweeps of a forward enqueued without a host read per sweep ------------
    def loop_begin(self):
        check(lib().pdp_loop_begin(self._h, _stream()))

    def loop_step(self, active_mask):
        check(lib().pdp_loop_step(self._h, ptr(active_mask, torch.uint8, self.B, 'active_mask'), _stream()))

    def loop_read(self, end=False):
        "(stopped, executed sweeps); waits for the stream"
        stopped, iters = C.c_int32(0), C.c_int32(0)
        check(lib().pdp_loop_read(self._h, C.byref(stopped), C.byref(iters), C.c_int(1 if end else 0), _stream()))
        return bool(stopped.value), int(iters.value)

    # -- decimators --------------------------------------------------------------------------------------------
    def sequential_decimate(self, dec, fs, active_mask, tolerance, t_max, pi=0.0):
        check(lib().pdp_sequential_decimate(self._h, dec._h, ptr(fs, torch.float32, 2 * self.E, 'message_state[1]'),
                                            ptr(active_mask, torch.uint8, self.B, 'active_mask'), C.c_float(tolerance),
                                            C.c_float(t_max), C.c_float(pi), _stream()))

    def sequential_decimate_gate(self, dec, fs, active_mask, tolerance, t_max):
        flag = C.c_int32(0)
        check(lib().pdp_sequential_decimate_gate(self._h, dec._h, ptr(fs, torch.float32, 2 * self.E), ptr(active_mask, torch.uint8, self.B),
                                                 C.c_float(tolerance), C.c_float(t_max), C.byref(flag), _stream()))
        return bool(flag.value)

    def sequential_decimate_apply(self, dec, fs, score, active_mask):
        check(lib().pdp_sequential_decimate_apply(self._h, dec._h, ptr(fs, torch.float32, 2 * self.E),
                                                  ptr(score, torch.float32, self.V), ptr(active_mask, torch.uint8, self.B), _stream()))

    def reinforce_decimate(self, dec, fs, active_mask, coin, decimation_probability, pi):
        check(lib().pdp_reinforce_decimate(self._h, dec._h, ptr(fs, torch.float32, 2 * self.E), ptr(active_mask, torch.uint8, self.B),
                                           C.c_float(coin), C.c_float(decimation_probability), C.c_float(pi), _stream()))

    def reinforce_predict(self, fs):
        out = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_reinforce_predict(self._h, ptr(fs, torch.float32, 2 * self.E), ptr(out), _stream()))
        return out

    # -- complete solver ---------------------------------------------------------------------------------------
    def exact_solve(self, budget=0, hints=None, learn=False, arena=0, stats=False):
        """Label every instance with the batched DPLL solver (pdp_exact_solve): (status int8 [B]: 1 SAT, 0 UNSAT, -1 undecided within
        ``budget`` clause-literal reads per instance, 0 = the library default; model float [V]: a satisfying 0/1 assignment of every status-1
        instance, 0 elsewhere; work int64 [B]: the clause-literal reads of each search).  Asynchronous on the current stream.
        ``hints`` (float32, V elements, on the problem's device): phase hints, pdp_exact_solve_hinted -- > 0.5 true first, other finite values
        false first, NaN no hint; an instance whose hints are all finite and satisfy it is answered by one pass over its clauses.
        ``learn``: the search with conflict clause learning and backjumping (pdp_exact_solve_learn), with ``arena`` words per instance for
        learned clauses (0: four per literal of the instance).  ``stats`` (learning search only): also return learned int32 [B], the clauses
        each instance learned."""
        if isinstance(arena, bool) or not isinstance(arena, numbers.Integral) or not 0 <= arena <= 1 << 30:
            raise ValueError("arena must be an integer from 0 to 2^30 words, got %r" % (arena,))
        if (arena or stats) and not learn:
            raise ValueError("arena and stats belong to the learning search: pass learn=True")
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable), got %s"
                                 % (self.V, '%s of %d' % (hints.dtype, hints.numel()) if torch.is_tensor(hints) else type(hints).__name__))
            hints = hints.reshape(-1).contiguous()
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        if learn:
            learned = torch.empty(self.B, dtype=torch.int32, device=self.device)
            check(lib().pdp_exact_solve_learn(self._h, ptr(hints, torch.float32, self.V, 'hints'), C.c_int64(int(budget)), C.c_int64(int(arena)),
                                              ptr(status), ptr(model), ptr(work), ptr(learned), _stream()))
            return (status, model, work, learned) if stats else (status, model, work)
        if hints is None:
            check(lib().pdp_exact_solve(self._h, C.c_int64(int(budget)), ptr(status), ptr(model), ptr(work), _stream()))
        else:
            check(lib().pdp_exact_solve_hinted(self._h, ptr(hints, torch.float32, self.V, 'hints'), C.c_int64(int(budget)), ptr(status), ptr(model),
                                               ptr(work), _stream()))
        return status, model, work

    def exact_solve_split(self, budget=0, hints=None, depth=None, stats=False):
        """exact_solve(hints) with the search of instance b spread over 2^depth[b] waves (pdp_exact_solve_split): (status, model, work) as
        exact_solve's -- status and model equal its bit for bit while no cube runs out of ``budget``, which applies to every cube; work is
        the sum over the cubes that count.  ``depth``: an int, or an int8 tensor of B elements on the problem's device, values 0 .. 16, at
        most 2^22 cubes per call; None: 0.  ``stats``: also first int32 [B] (the lowest cube with a model, -1: none, or the hints were
        accepted as a whole), depth_used int8 [B] (0 for an instance on the HBM route), cube_off int64 [B+1], cube_status int8 [cubes]
        (1 / 0 / -1, -2: stopped because a lower cube had answered) and cube_work int64 [cubes]; the records of cubes above first depend
        on timing, nothing else does.  Synchronises the current stream once, then asynchronous on it (``stats`` synchronises again)."""
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable), got %s"
                                 % (self.V, '%s of %d' % (hints.dtype, hints.numel()) if torch.is_tensor(hints) else type(hints).__name__))
            hints = hints.reshape(-1).contiguous()
        if depth is None:
            depth = 0
        if torch.is_tensor(depth):
            if depth.dtype != torch.int8 or depth.numel() != self.B or depth.device != self.device:
                raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance) on %s, got %s of %d on %s"
                                 % (self.B, self.device, depth.dtype, depth.numel(), depth.device))
            depth = depth.reshape(-1).contiguous()
        elif isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not -128 <= depth <= 127:
            raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance), got %r" % (self.B, depth))
        else:
            depth = torch.full((self.B,), int(depth), dtype=torch.int8, device=self.device)
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        first = torch.empty(self.B, dtype=torch.int32, device=self.device)
        depth_used = torch.empty(self.B, dtype=torch.int8, device=self.device)
        check(lib().pdp_exact_solve_split(self._h, ptr(hints, torch.float32, self.V, 'hints'), ptr(depth), C.c_int64(int(budget)), ptr(status),
                                          ptr(model), ptr(work), ptr(first), ptr(depth_used), _stream()))
        if not stats:
            return status, model, work
        cubes = int(torch.bitwise_left_shift(torch.ones_like(depth_used, dtype=torch.int64), depth_used.to(torch.int64)).sum().item())
        cube_off = torch.empty(self.B + 1, dtype=torch.int64, device=self.device)
        cube_status = torch.empty(cubes, dtype=torch.int8, device=self.device)
        cube_work = torch.empty(cubes, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_split_cubes(self._h, ptr(cube_off), ptr(cube_status), ptr(cube_work), _stream()))
        return status, model, work, first, depth_used, cube_off, cube_status, cube_work

    def exact_min_unsat(self, budget=0, hints=None, stats=False):
        """The fewest unsatisfied clauses of every instance by branch and bound (pdp_exact_min_unsat): (status int8 [B]: 1 the cost is the
        minimum over all assignments, -1 the budget ran out and it is an upper bound; cost int32 [B]: the clauses the model leaves
        unsatisfied; model float [V]: a complete 0/1 assignment; work int64 [B]), plus improvements int32 [B] with ``stats``: how often the
        incumbent was replaced.  ``hints`` (float32, V elements, as in exact_solve): the first incumbent, > 0.5 true and every other value
        false, NaN included; None: all false.  ``budget`` as in exact_solve.  Asynchronous on the current stream."""
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable), got %s"
                                 % (self.V, '%s of %d' % (hints.dtype, hints.numel()) if torch.is_tensor(hints) else type(hints).__name__))
            hints = hints.reshape(-1).contiguous()
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        cost = torch.empty(self.B, dtype=torch.int32, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        improvements = torch.empty(self.B, dtype=torch.int32, device=self.device)
        check(lib().pdp_exact_min_unsat(self._h, ptr(hints, torch.float32, self.V, 'hints'), C.c_int64(int(budget)), ptr(status), ptr(cost),
                                        ptr(model), ptr(work), ptr(improvements), _stream()))
        return (status, cost, model, work, improvements) if stats else (status, cost, model, work)

    def exact_nearest(self, hints=None, penalties=None, budget=0, stats=False):
        """The model of every instance nearest to ``hints`` (pdp_exact_nearest): (status int8 [B]: 1 cost is the minimum over the models
        and model attains it, 0 the instance has no model, -1 the budget ran out and cost / model are the best model met so far, cost -1
        and model all 0 if none was, -3 a penalty of the instance is outside [0, 2^20] and it was not searched; cost int64 [B]: the sum of
        the penalties of the variables where model differs from the thresholded hints; model float32 [V]; work int64 [B]), plus
        improvements int32 [B] with ``stats``: how often a better model was met.  ``hints`` (float32, V elements, on the problem's
        device): > 0.5 true and every other value false, NaN included; None: all false.  ``penalties`` (int32, V elements, on the
        problem's device): what a variable costs where it differs; None: all 1, the Hamming distance.  ``budget`` as in exact_solve.
        Asynchronous on the current stream."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        for name, t, dtype in (('hints', hints, torch.float32), ('penalties', penalties, torch.int32)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != self.V:
                raise ValueError("%s must be a %s tensor of %d elements (one per variable), got %s"
                                 % (name, dtype, self.V, '%s of %d' % (t.dtype, t.numel()) if torch.is_tensor(t) else type(t).__name__))
            if t.device != self.device:
                raise ValueError("%s must live on %s, got %s" % (name, self.device, t.device))
        if hints is not None:
            hints = hints.reshape(-1).contiguous()
        if penalties is not None:
            penalties = penalties.reshape(-1).contiguous()
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        cost = torch.empty(self.B, dtype=torch.int64, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        improvements = torch.empty(self.B, dtype=torch.int32, device=self.device)
        check(lib().pdp_exact_nearest(self._h, ptr(hints, torch.float32, self.V, 'hints'), ptr(penalties, torch.int32, self.V, 'penalties'),
                                      C.c_int64(int(budget)), ptr(status), ptr(cost), ptr(model), ptr(work), ptr(improvements), _stream()))
        return (status, cost, model, work, improvements) if stats else (status, cost, model, work)

    def exact_min_unsat_split(self, budget=0, hints=None, depth=None, stats=False):
        """exact_min_unsat(hints) with the search of instance b spread over 2^depth[b] waves that share the best cost found so far
        (pdp_exact_min_unsat_split): (status, cost, model, work) as exact_min_unsat's.  With a ``budget`` -- it applies to every cube -- that
        no cube exhausts, status is 1 and cost the minimum, and model attains cost at any budget; at depth 0 all outputs are
        exact_min_unsat's bit for bit.  Above depth 0, which minimiser model is, work, and the ``stats`` other than depth_used and cube_off
        depend on which cube lowers the shared cost first, unless one wave runs all cubes (PDP_EXACT_GRID=1).  ``depth``: an int, or an int8
        tensor of B elements on the problem's device, values 0 .. 16, at most 2^22 cubes per call; None: 0.  ``stats``: also improvements
        int32 [B], first int32 [B] (the lowest cube that holds the cost, -1: the thresholded hints do), depth_used int8 [B] (0 for an
        instance on the HBM route), cube_off int64 [B+1], cube_status int8 [cubes] (1 exhausted / -1 budget spent), cube_cost int32 [cubes]
        (the cube's last accepted cost, -1: none), cube_work int64 [cubes] and cube_improvements int32 [cubes].  Synchronises the current
        stream once, then asynchronous on it (``stats`` synchronises again)."""
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable), got %s"
                                 % (self.V, '%s of %d' % (hints.dtype, hints.numel()) if torch.is_tensor(hints) else type(hints).__name__))
            hints = hints.reshape(-1).contiguous()
        if depth is None:
            depth = 0
        if torch.is_tensor(depth):
            if depth.dtype != torch.int8 or depth.numel() != self.B or depth.device != self.device:
                raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance) on %s, got %s of %d on %s"
                                 % (self.B, self.device, depth.dtype, depth.numel(), depth.device))
            depth = depth.reshape(-1).contiguous()
        elif isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not -128 <= depth <= 127:
            raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance), got %r" % (self.B, depth))
        else:
            depth = torch.full((self.B,), int(depth), dtype=torch.int8, device=self.device)
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        cost = torch.empty(self.B, dtype=torch.int32, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        improvements = torch.empty(self.B, dtype=torch.int32, device=self.device)
        first = torch.empty(self.B, dtype=torch.int32, device=self.device)
        depth_used = torch.empty(self.B, dtype=torch.int8, device=self.device)
        check(lib().pdp_exact_min_unsat_split(self._h, ptr(hints, torch.float32, self.V, 'hints'), ptr(depth), C.c_int64(int(budget)), ptr(status),
                                              ptr(cost), ptr(model), ptr(work), ptr(improvements), ptr(first), ptr(depth_used), _stream()))
        if not stats:
            return status, cost, model, work
        cubes = int(torch.bitwise_left_shift(torch.ones_like(depth_used, dtype=torch.int64), depth_used.to(torch.int64)).sum().item())
        cube_off = torch.empty(self.B + 1, dtype=torch.int64, device=self.device)
        cube_status = torch.empty(cubes, dtype=torch.int8, device=self.device)
        cube_cost = torch.empty(cubes, dtype=torch.int32, device=self.device)
        cube_work = torch.empty(cubes, dtype=torch.int64, device=self.device)
        cube_improvements = torch.empty(cubes, dtype=torch.int32, device=self.device)
        check(lib().pdp_exact_min_unsat_split_cubes(self._h, ptr(cube_off), ptr(cube_status), ptr(cube_cost), ptr(cube_work),
                                                    ptr(cube_improvements), _stream()))
        return status, cost, model, work, improvements, first, depth_used, cube_off, cube_status, cube_cost, cube_work, cube_improvements

    def exact_nearest_split(self, hints=None, penalties=None, start=None, depth=None, budget=0, stats=False):
        """exact_nearest(hints, penalties) with the search of instance b spread over 2^depth[b] waves that share the cost of the best model
        found so far (pdp_exact_nearest_split): (status, cost, model, work) as exact_nearest's.  With a ``budget`` -- it applies to every
        cube -- that no cube exhausts, status and cost are exact_nearest's and model attains cost; at any budget cost is -1 or an upper
        bound that model attains; at depth 0 without ``start`` all outputs are exact_nearest's bit for bit.  ``start`` (float32, V elements,
        on the problem's device; None: none): a model of every instance the caller already has, thresholded like the hints; the kernel
        checks it and computes its distance itself, the search starts below that distance, and where it is not a model it is ignored.
        Above depth 0, which minimiser model is, work, and the ``stats`` other than depth_used, start_cost and cube_off depend on which cube
        lowers the shared cost first, unless one wave runs all cubes (PDP_EXACT_GRID=1).  ``depth``: an int, or an int8 tensor of B elements
        on the problem's device, values 0 .. 16, at most 2^22 cubes per call; None: 0.  ``stats``: also improvements int32 [B], first int32
        [B] (the lowest cube that holds the cost, -1: the hints or the start model do, or nothing does), depth_used int8 [B] (0 for an
        instance on the HBM route), start_cost int64 [B] (the distance of the start model, -1: none or not a model), cube_off int64 [B+1],
        cube_status int8 [cubes] (1 exhausted / -1 budget spent), cube_cost int64 [cubes] (the cube's last accepted cost, -1: none),
        cube_work int64 [cubes] and cube_improvements int32 [cubes].  Synchronises the current stream once, then asynchronous on it
        (``stats`` synchronises again)."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        for name, t, dtype in (('hints', hints, torch.float32), ('penalties', penalties, torch.int32), ('start', start, torch.float32)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != self.V:
                raise ValueError("%s must be a %s tensor of %d elements (one per variable), got %s"
                                 % (name, dtype, self.V, '%s of %d' % (t.dtype, t.numel()) if torch.is_tensor(t) else type(t).__name__))
            if t.device != self.device:
                raise ValueError("%s must live on %s, got %s" % (name, self.device, t.device))
        if hints is not None:
            hints = hints.reshape(-1).contiguous()
        if penalties is not None:
            penalties = penalties.reshape(-1).contiguous()
        if start is not None:
            start = start.reshape(-1).contiguous()
        if depth is None:
            depth = 0
        if torch.is_tensor(depth):
            if depth.dtype != torch.int8 or depth.numel() != self.B or depth.device != self.device:
                raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance) on %s, got %s of %d on %s"
                                 % (self.B, self.device, depth.dtype, depth.numel(), depth.device))
            depth = depth.reshape(-1).contiguous()
        elif isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not -128 <= depth <= 127:
            raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance), got %r" % (self.B, depth))
        else:
            depth = torch.full((self.B,), int(depth), dtype=torch.int8, device=self.device)
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        cost = torch.empty(self.B, dtype=torch.int64, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        improvements = torch.empty(self.B, dtype=torch.int32, device=self.device)
        first = torch.empty(self.B, dtype=torch.int32, device=self.device)
        depth_used = torch.empty(self.B, dtype=torch.int8, device=self.device)
        start_cost = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_nearest_split(self._h, ptr(hints, torch.float32, self.V, 'hints'), ptr(penalties, torch.int32, self.V, 'penalties'),
                                            ptr(start, torch.float32, self.V, 'start'), ptr(depth), C.c_int64(int(budget)), ptr(status),
                                            ptr(cost), ptr(model), ptr(work), ptr(improvements), ptr(first), ptr(depth_used), ptr(start_cost),
                                            _stream()))
        if not stats:
            return status, cost, model, work
        cubes = int(torch.bitwise_left_shift(torch.ones_like(depth_used, dtype=torch.int64), depth_used.to(torch.int64)).sum().item())
        cube_off = torch.empty(self.B + 1, dtype=torch.int64, device=self.device)
        cube_status = torch.empty(cubes, dtype=torch.int8, device=self.device)
        cube_cost = torch.empty(cubes, dtype=torch.int64, device=self.device)
        cube_work = torch.empty(cubes, dtype=torch.int64, device=self.device)
        cube_improvements = torch.empty(cubes, dtype=torch.int32, device=self.device)
        check(lib().pdp_exact_nearest_split_cubes(self._h, ptr(cube_off), ptr(cube_status), ptr(cube_cost), ptr(cube_work),
                                                  ptr(cube_improvements), _stream()))
        return (status, cost, model, work, improvements, first, depth_used, start_cost, cube_off, cube_status, cube_cost, cube_work,
                cube_improvements)

    def exact_count(self, budget=0, stats=False):
        """Exact model counts and per-variable counts of every instance (pdp_exact_count): (status int8 [B]: 1 the search is complete and
        count is the number of models, -1 the budget ran out and count covers the part of the tree visited so far, a lower bound, -2 the
        instance has more than 1023 variables and was not searched; count float64 [B]; true_count float64 [V]: the models among those
        counted in which the variable is true; work int64 [B]), plus leaves int64 [B] with ``stats``: the satisfying cubes met.  An
        unsatisfiable instance is status 1 with count 0.  While count <= 2^53 every value is an exact integer.  ``budget`` as in
        exact_solve.  Asynchronous on the current stream."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        count = torch.empty(self.B, dtype=torch.float64, device=self.device)
        true_count = torch.empty(self.V, dtype=torch.float64, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        leaves = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_count(self._h, C.c_int64(int(budget)), ptr(status), ptr(count), ptr(true_count), ptr(work), ptr(leaves),
                                    _stream()))
        return (status, count, true_count, work, leaves) if stats else (status, count, true_count, work)

    def exact_mass(self, weights, budget=0, stats=False):
        """The exact solution mass of a soft prediction (pdp_exact_mass): with ``weights`` (float32, V elements, contiguous, on the
        problem's device) as independent probabilities of the variables being true, (status int8 [B]: 1 the search is complete and mass
        is the probability that such a draw is a model, -1 the budget ran out and that probability lies in [mass, mass + open_mass], -2
        more than 1023 variables, -3 a weight of the instance is NaN or outside [0, 1], neither searched; mass float64 [B]; true_mass
        float64 [V]: the part of mass with the variable true, so true_mass / mass is the posterior; open_mass float64 [B]: the mass of
        the part of the tree not yet visited, 0 at status 1; work int64 [B]), plus leaves int64 [B] with ``stats``.  An unsatisfiable
        instance is status 1 with mass 0.  ``budget`` as in exact_solve.  Asynchronous on the current stream."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        if not torch.is_tensor(weights):
            raise NativeError("weights must be a float32 tensor of %d elements on %s, got %s" % (self.V, self.device, type(weights).__name__))
        if weights.device != self.device:
            raise NativeError("weights must live on %s, got %s" % (self.device, weights.device))
        weights = ptr(weights, torch.float32, self.V, 'weights')
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        mass = torch.empty(self.B, dtype=torch.float64, device=self.device)
        true_mass = torch.empty(self.V, dtype=torch.float64, device=self.device)
        open_mass = torch.empty(self.B, dtype=torch.float64, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        leaves = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_mass(self._h, weights, C.c_int64(int(budget)), ptr(status), ptr(mass), ptr(true_mass), ptr(open_mass), ptr(work),
                                   ptr(leaves), _stream()))
        return (status, mass, true_mass, open_mass, work, leaves) if stats else (status, mass, true_mass, open_mass, work)

    def exact_count_split(self, budget=0, depth=None, stats=False):
        """exact_count with the search of instance b spread over 2^depth[b] waves (pdp_exact_count_split): (status, count, true_count, work)
        as exact_count's -- count and true_count equal its bit for bit while count <= 2^53 and no cube runs out of ``budget``, which applies
        to every cube; work is the sum over the cubes.  ``depth``: an int, or an int8 tensor of B elements on the problem's device, values
        0 .. 16, at most 2^22 cubes and 2^31 bytes of per-cube rows per call; None: 0.  ``stats``: also leaves int64 [B], depth_used int8
        [B] (0 for an instance on the HBM route or of more than 1023 variables), cube_off int64 [B+1], cube_status int8 [cubes], cube_count
        float64 [cubes], cube_work and cube_leaves int64 [cubes].  Everything is a function of the instances, the depths and the budget.
        Synchronises the current stream once, then asynchronous on it (``stats`` synchronises again)."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        if depth is None:
            depth = 0
        if torch.is_tensor(depth):
            if depth.dtype != torch.int8 or depth.numel() != self.B or depth.device != self.device:
                raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance) on %s, got %s of %d on %s"
                                 % (self.B, self.device, depth.dtype, depth.numel(), depth.device))
            depth = depth.reshape(-1).contiguous()
        elif isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not -128 <= depth <= 127:
            raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance), got %r" % (self.B, depth))
        else:
            depth = torch.full((self.B,), int(depth), dtype=torch.int8, device=self.device)
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        count = torch.empty(self.B, dtype=torch.float64, device=self.device)
        true_count = torch.empty(self.V, dtype=torch.float64, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        leaves = torch.empty(self.B, dtype=torch.int64, device=self.device)
        depth_used = torch.empty(self.B, dtype=torch.int8, device=self.device)
        check(lib().pdp_exact_count_split(self._h, ptr(depth), C.c_int64(int(budget)), ptr(status), ptr(count), ptr(true_count), ptr(work),
                                          ptr(leaves), ptr(depth_used), _stream()))
        if not stats:
            return status, count, true_count, work
        cubes = int(torch.bitwise_left_shift(torch.ones_like(depth_used, dtype=torch.int64), depth_used.to(torch.int64)).sum().item())
        cube_off = torch.empty(self.B + 1, dtype=torch.int64, device=self.device)
        cube_status = torch.empty(cubes, dtype=torch.int8, device=self.device)
        cube_count = torch.empty(cubes, dtype=torch.float64, device=self.device)
        cube_work = torch.empty(cubes, dtype=torch.int64, device=self.device)
        cube_leaves = torch.empty(cubes, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_count_split_cubes(self._h, ptr(cube_off), ptr(cube_status), ptr(cube_count), ptr(cube_work), ptr(cube_leaves),
                                                _stream()))
        return status, count, true_count, work, leaves, depth_used, cube_off, cube_status, cube_count, cube_work, cube_leaves

    def exact_count_begin(self):
        """The state of a resumable count (pdp_exact_count_round): the root frontier -- one cube of length 0 per instance of at most 1023
        variables -- zeroed totals, and status -1 (open), or -2 where the instance is not searched.  See CountState."""
        words = C.c_int32()
        check(lib().pdp_exact_count_frontier_words(self._h, C.byref(words)))
        dev = self.device
        n = torch.bincount(self.export_graph()[1].to(torch.int64), minlength=self.B)[:self.B]
        wide = n > COUNT_ROUNDS_MAX_N
        cube_off = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
        cube_off[1:] = torch.cumsum((~wide).to(torch.int64), 0)
        cubes = int(cube_off[-1].item())
        s = CountState()
        s.cube_off = cube_off
        s.len = torch.zeros(cubes, dtype=torch.int32, device=dev)
        s.bits = torch.zeros(cubes, words.value, dtype=torch.int32, device=dev)
        s.closed = torch.zeros(cubes, words.value, dtype=torch.int32, device=dev)
        s.count = torch.zeros(self.B, dtype=torch.float64, device=dev)
        s.true_count = torch.zeros(self.V, dtype=torch.float64, device=dev)
        s.work = torch.zeros(self.B, dtype=torch.int64, device=dev)
        s.leaves = torch.zeros(self.B, dtype=torch.int64, device=dev)
        s.rounds = torch.zeros(self.B, dtype=torch.int32, device=dev)
        s.status = torch.where(wide, -2, -1).to(torch.int8)
        return s

    def exact_count_round(self, state, budget=0, give=0, stats=False):
        """One round of a resumable count (pdp_exact_count_round, then pdp_exact_count_expand): every open cube of ``state`` runs for
        ``budget`` clause-literal reads past the replay of its path (0: the library default, 2^18), the totals of the state take what it
        counted, and the frontier becomes the checkpoints of the cubes that stopped, each cut into up to ``give`` children and a remainder.
        Advances ``state`` in place and returns the number of open cubes; 0: the count is complete, and while count <= 2^53 the totals equal
        exact_count's bit for bit, whatever the budgets and gives of the rounds were.  ``stats``: also the round's per-cube records
        (cube_off int64 [B+1] of the frontier that ran, cube_status int8 [cubes] 1 / -1, cube_count float64, cube_work, cube_leaves and
        cube_replay int64 [cubes], and the checkpoints len_out int32 [cubes], bits_out and closed_out int32 [cubes, words]).  The state
        may come from another Problem of the same items.  A malformed state raises before anything is searched or written.  More than
        2^22 cubes after the expansion raises; lower ``give``.  Synchronises the current stream twice."""
        self._round_args(state, CountState, 'exact_count_begin', budget, give)
        dev = self.device
        cubes = state.cubes
        cube_status, len_out, bits_out, closed_out = out = self._round_buffers(state)
        rec = [torch.empty(cubes, dtype=torch.float64 if k == 0 else torch.int64, device=dev) if stats else None for k in range(4)]
        check(lib().pdp_exact_count_round(self._h, ptr(state.cube_off), C.c_int64(cubes), ptr(state.len), ptr(state.bits), ptr(state.closed),
                                          C.c_int64(int(budget)), ptr(state.count), ptr(state.true_count), ptr(state.work), ptr(state.leaves),
                                          ptr(cube_status), ptr(len_out), ptr(bits_out), ptr(closed_out), ptr(rec[0]), ptr(rec[1]),
                                          ptr(rec[2]), ptr(rec[3]), _stream()))
        made, ran = self._round_expand(state, *out, give)
        open_ = state.cube_off[1:] > state.cube_off[:-1]
        state.status = torch.where(state.status == -2, state.status, torch.where(open_, -1, 1).to(torch.int8))
        if not stats:
            return made
        return made, (ran, cube_status, rec[0], rec[1], rec[2], rec[3], len_out, bits_out, closed_out)

    def _round_args(self, state, cls, begin_name, budget, give):
        "the refusals every round call makes before anything runs"
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads per cube (0: the library default), got %r" % (budget,))
        if isinstance(give, bool) or not isinstance(give, numbers.Integral) or not 0 <= give <= COUNT_ROUNDS_MAX_N:
            raise ValueError("give must be an integer from 0 to %d, got %r" % (COUNT_ROUNDS_MAX_N, give))
        if not isinstance(state, cls):
            raise ValueError("state must come from %s, got %s" % (begin_name, type(state).__name__))
        state.validate(self)

    def _round_buffers(self, state):
        "what every round writes per cube: (cube_status, len_out, bits_out, closed_out), the checkpoints shaped as the frontier"
        dev = self.device
        cubes, words = int(state.len.numel()), int(state.bits.size(1))
        return (torch.empty(cubes, dtype=torch.int8, device=dev), torch.empty(cubes, dtype=torch.int32, device=dev),
                torch.empty(max(cubes, 1), words, dtype=torch.int32, device=dev)[:cubes],
                torch.empty(max(cubes, 1), words, dtype=torch.int32, device=dev)[:cubes])

    def _round_expand(self, state, cube_status, len_out, bits_out, closed_out, give):
        """The tail of every round (pdp_exact_count_expand): the checkpoints of the cubes that stopped become the state's frontier, each
        cut into up to ``give`` children and a remainder.  Returns (open cubes, the cube_off of the frontier that ran)."""
        dev = self.device
        cubes, words = int(state.len.numel()), int(state.bits.size(1))
        capacity = min(cubes * (1 + int(give)), COUNT_ROUNDS_MAX_CUBES)
        cube_off = torch.empty(self.B + 1, dtype=torch.int64, device=dev)
        len_new = torch.empty(capacity, dtype=torch.int32, device=dev)
        bits_new = torch.empty(max(capacity, 1), words, dtype=torch.int32, device=dev)
        closed_new = torch.empty(max(capacity, 1), words, dtype=torch.int32, device=dev)
        made = C.c_int64()
        ran = state.cube_off
        check(lib().pdp_exact_count_expand(self._h, ptr(ran), C.c_int64(cubes), ptr(cube_status), ptr(len_out), ptr(bits_out), ptr(closed_out),
                                           C.c_int32(int(give)), C.c_int64(capacity), ptr(cube_off), ptr(len_new), ptr(bits_new),
                                           ptr(closed_new), C.byref(made), _stream()))
        made = int(made.value)
        state.rounds += (ran[1:] > ran[:-1]).to(torch.int32)
        state.cube_off, state.len, state.bits, state.closed = cube_off, len_new[:made], bits_new[:made], closed_new[:made]
        return made, ran

    def exact_solve_begin(self, hints=None):
        """The state of a resumable deciding search (pdp_exact_solve_round): the root frontier -- one cube of length 0 per instance of at
        most 1023 variables -- status -1 (open), or -2 where the instance is not searched, zeroed models and work.  ``hints`` (float32, V
        elements, on the problem's device; None: none) are kept on the state and steer every round.  See SolveState."""
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V or hints.device != self.device:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable) on %s, got %s"
                                 % (self.V, self.device, '%s of %d on %s' % (hints.dtype, hints.numel(), hints.device)
                                    if torch.is_tensor(hints) else type(hints).__name__))
        c = self.exact_count_begin()
        s = SolveState()
        s.cube_off, s.len, s.bits, s.closed, s.status, s.work, s.rounds = c.cube_off, c.len, c.bits, c.closed, c.status, c.work, c.rounds
        s.hint = (torch.full((self.V,), float('nan'), dtype=torch.float32, device=self.device) if hints is None
                  else hints.reshape(-1).contiguous().clone())
        s.model = torch.zeros(self.V, dtype=torch.float32, device=self.device)
        return s

    def exact_solve_round(self, state, budget=0, give=0, stats=False):
        """One round of a resumable deciding search (pdp_exact_solve_round, then pdp_exact_count_expand): every open cube of ``state`` runs
        for ``budget`` clause-literal reads past the replay of its path (0: the library default); an instance one of whose cubes found a
        model becomes status 1 with that model and leaves the frontier, one whose cubes all ended without one becomes 0, and the
        checkpoints of the others are cut into up to ``give`` children and a remainder each.  Advances ``state`` in place and returns the
        number of open cubes.  Once decided, status is exact_solve's; with ``give`` 0 throughout, status and model are exact_solve's with
        the state's hints bit for bit wherever its check pass does not accept them; with more, which model comes back is not promised.
        ``stats``: also the round's records (cube_off int64 [B+1] of the frontier that ran, cube_status int8 [cubes] 1 / 0 / -1 / -2
        dropped, cube_work and cube_replay int64 [cubes], the checkpoints len_out int32 [cubes], bits_out and closed_out int32 [cubes,
        words], and first int32 [B]: the instance's lowest cube that answered 1, -1 none).  The state may come from another Problem of the
        same items.  A malformed state raises before anything is searched or written.  More than 2^22 cubes after the expansion raises;
        lower ``give``.  Synchronises the current stream twice."""
        self._round_args(state, SolveState, 'exact_solve_begin', budget, give)
        dev = self.device
        cubes = state.cubes
        cube_status, len_out, bits_out, closed_out = out = self._round_buffers(state)
        first = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        rec = [torch.empty(cubes, dtype=torch.int64, device=dev) if stats else None for _ in range(2)]
        check(lib().pdp_exact_solve_round(self._h, ptr(state.hint), ptr(state.cube_off), C.c_int64(cubes), ptr(state.len), ptr(state.bits),
                                          ptr(state.closed), C.c_int64(int(budget)), ptr(state.status), ptr(state.model), ptr(state.work),
                                          ptr(first), ptr(cube_status), ptr(len_out), ptr(bits_out), ptr(closed_out), ptr(rec[0]),
                                          ptr(rec[1]), _stream()))
        made, ran = self._round_expand(state, *out, give)
        if not stats:
            return made
        return made, (ran, cube_status, rec[0], rec[1], len_out, bits_out, closed_out, first)

    def exact_nearest_begin(self, hints=None, penalties=None, start=None):
        """The state of a resumable nearest-model search (pdp_exact_nearest_round): the root frontier -- one cube of length 0 per instance
        of at most 1023 variables whose penalties all lie in [0, 2^20] -- status -1 (open), -2 where the instance is not searched or -3
        where a penalty is out of range, cost -1, zeroed models, work and improvements.  ``hints`` (float32, V elements, on the problem's
        device; None: all false) and ``penalties`` (int32, V elements; None: all 1) are kept on the state and used by every round.
        ``start`` (float32, V elements; None: none): a model of every instance the caller already has, thresholded like the hints.  It is
        checked, not trusted: its unsatisfied clauses are counted by cnf_eval on this handle and its distance is summed in int64, and
        only where it is a model of an instance that has a cube does it seed cost and model.  See NearestState."""
        for name, t, dtype in (('hints', hints, torch.float32), ('penalties', penalties, torch.int32), ('start', start, torch.float32)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != self.V or t.device != self.device:
                raise ValueError("%s must be a %s tensor of %d elements (one per variable) on %s, got %s"
                                 % (name, dtype, self.V, self.device,
                                    '%s of %d on %s' % (t.dtype, t.numel(), t.device) if torch.is_tensor(t) else type(t).__name__))
        dev = self.device
        c = self.exact_count_begin()
        s = NearestState()
        s.hint = torch.zeros(self.V, dtype=torch.float32, device=dev) if hints is None else hints.reshape(-1).contiguous().clone()
        s.penalty = torch.ones(self.V, dtype=torch.int32, device=dev) if penalties is None else penalties.reshape(-1).contiguous().clone()
        owner = self.export_graph()[1].to(torch.int64).reshape(-1)                # the instance of every variable
        out_of_range = ((s.penalty < 0) | (s.penalty > EXACT_NEAREST_MAX_PENALTY)).to(torch.int64)
        bad = torch.zeros(self.B, dtype=torch.int64, device=dev).index_add_(0, owner, out_of_range) > 0
        s.status = torch.where(bad, torch.full_like(c.status, -3), c.status)
        has = s.status == -1
        s.cube_off = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
        s.cube_off[1:] = torch.cumsum(has.to(torch.int64), 0)
        cubes = int(s.cube_off[-1].item())
        s.len, s.bits, s.closed = c.len[:cubes].clone(), c.bits[:cubes].clone(), c.closed[:cubes].clone()
        s.cost = torch.full((self.B,), -1, dtype=torch.int64, device=dev)
        s.model = torch.zeros(self.V, dtype=torch.float32, device=dev)
        s.work, s.rounds = c.work, c.rounds
        s.improvements = torch.zeros(self.B, dtype=torch.int32, device=dev)
        if start is not None:
            x = (start.reshape(-1) > 0.5)
            unsat = self.cnf_eval(x.to(torch.float32).contiguous())[1].reshape(-1)
            differs = (x != (s.hint > 0.5)).to(torch.int64) * s.penalty.to(torch.int64)
            far = torch.zeros(self.B, dtype=torch.int64, device=dev).index_add_(0, owner, differs)
            seeded = has & (unsat == 0)
            s.cost = torch.where(seeded, far, s.cost)
            s.model = torch.where(seeded[owner], x.to(torch.float32), s.model)
        return s

    def exact_nearest_round(self, state, budget=0, give=0, stats=False):
        """One round of a resumable nearest-model search (pdp_exact_nearest_round, then pdp_exact_count_expand): every open cube of
        ``state`` runs for ``budget`` clause-literal reads past the replay of its path (0: the library default) under the bound
        state.cost of its instance as it stands when the round begins; the instance takes the minimum of its cubes' costs and the model
        of the lowest cube that holds it, so the next round hands every cube the best bound any of them found.  An instance that reaches
        cost 0, or whose cubes have all ended, becomes status 1 (0 where no model was ever met) and leaves the frontier; the checkpoints of
        the others are cut into up to ``give`` children and a remainder each.  Advances ``state`` in place and returns the number of
        open cubes.  After every round cost is -1 or attained by model, and it never rises.  Once the frontier is empty, status and cost
        are exact_nearest's; with ``give`` 0 throughout so are model and improvements, bit for bit, wherever its check pass does not
        accept the hints (where it does: cost 0, model = the thresholded hints, one improvement).  Every output is a function of the
        state, ``budget`` and ``give`` alone.  ``stats``: also the round's records (cube_off int64 [B+1] of the frontier that ran,
        cube_status int8 [cubes] 1 ended / -1 stopped / -2 dropped, cube_cost int64 [cubes] (-1: none), cube_work and cube_replay int64
        [cubes], cube_improvements int32 [cubes], the checkpoints len_out int32 [cubes], bits_out and closed_out int32 [cubes, words],
        and first int32 [B]: the instance's lowest cube that holds its new cost, -1: the cost did not fall).  The state may come from
        another Problem of the same items.  A malformed state, or a penalty out of range on an instance that has a cube, raises before
        anything is searched or written.  More than 2^22 cubes after the expansion raises; lower ``give``.  Synchronises the current
        stream twice."""
        self._round_args(state, NearestState, 'exact_nearest_begin', budget, give)
        dev = self.device
        cubes = state.cubes
        cube_status, len_out, bits_out, closed_out = out = self._round_buffers(state)
        first = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        rec = [torch.empty(cubes, dtype=torch.int64, device=dev) if stats else None for _ in range(3)]
        rec_imp = torch.empty(cubes, dtype=torch.int32, device=dev) if stats else None
        check(lib().pdp_exact_nearest_round(self._h, ptr(state.hint), ptr(state.penalty), ptr(state.cube_off), C.c_int64(cubes), ptr(state.len),
                                            ptr(state.bits), ptr(state.closed), C.c_int64(int(budget)), ptr(state.status), ptr(state.cost),
                                            ptr(state.model), ptr(state.work), ptr(state.improvements), ptr(first), ptr(cube_status),
                                            ptr(len_out), ptr(bits_out), ptr(closed_out), ptr(rec[0]), ptr(rec[1]), ptr(rec[2]), ptr(rec_imp),
                                            _stream()))
        made, ran = self._round_expand(state, *out, give)
        if not stats:
            return made
        return made, (ran, cube_status, rec[0], rec[1], rec[2], rec_imp, len_out, bits_out, closed_out, first)

    def exact_mass_split(self, weights, budget=0, depth=None, stats=False):
        """exact_mass with the search of instance b spread over 2^depth[b] waves (pdp_exact_mass_split): (status, mass, true_mass,
        open_mass, work) as exact_mass's.  ``budget`` applies to every cube; at status -1 the probability lies in [mass, mass + open_mass];
        work is the sum over the cubes.  With weights whose products are exact (small dyadic fractions) mass and true_mass equal
        exact_mass's bit for bit, elsewhere to the last bits.  ``weights`` as exact_mass's; ``depth``: an int, or an int8 tensor of B
        elements on the problem's device, values 0 .. 16, at most 2^22 cubes and 2^31 bytes of per-cube rows per call; None: 0.
        ``stats``: also leaves int64 [B], depth_used int8 [B] (0 for an instance on the HBM route or of more than 1023 variables),
        cube_off int64 [B+1], cube_status int8 [cubes], cube_mass and cube_open float64 [cubes], cube_work and cube_leaves int64 [cubes].
        Everything is a function of the instances, the weights, the depths and the budget.  Synchronises the current stream once, then
        asynchronous on it (``stats`` synchronises again)."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        if not torch.is_tensor(weights):
            raise NativeError("weights must be a float32 tensor of %d elements on %s, got %s" % (self.V, self.device, type(weights).__name__))
        if weights.device != self.device:
            raise NativeError("weights must live on %s, got %s" % (self.device, weights.device))
        weights = ptr(weights, torch.float32, self.V, 'weights')
        if depth is None:
            depth = 0
        if torch.is_tensor(depth):
            if depth.dtype != torch.int8 or depth.numel() != self.B or depth.device != self.device:
                raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance) on %s, got %s of %d on %s"
                                 % (self.B, self.device, depth.dtype, depth.numel(), depth.device))
            depth = depth.reshape(-1).contiguous()
        elif isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not -128 <= depth <= 127:
            raise ValueError("depth must be an int or an int8 tensor of %d elements (one per instance), got %r" % (self.B, depth))
        else:
            depth = torch.full((self.B,), int(depth), dtype=torch.int8, device=self.device)
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        mass = torch.empty(self.B, dtype=torch.float64, device=self.device)
        true_mass = torch.empty(self.V, dtype=torch.float64, device=self.device)
        open_mass = torch.empty(self.B, dtype=torch.float64, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        leaves = torch.empty(self.B, dtype=torch.int64, device=self.device)
        depth_used = torch.empty(self.B, dtype=torch.int8, device=self.device)
        check(lib().pdp_exact_mass_split(self._h, weights, ptr(depth), C.c_int64(int(budget)), ptr(status), ptr(mass), ptr(true_mass),
                                         ptr(open_mass), ptr(work), ptr(leaves), ptr(depth_used), _stream()))
        if not stats:
            return status, mass, true_mass, open_mass, work
        cubes = int(torch.bitwise_left_shift(torch.ones_like(depth_used, dtype=torch.int64), depth_used.to(torch.int64)).sum().item())
        cube_off = torch.empty(self.B + 1, dtype=torch.int64, device=self.device)
        cube_status = torch.empty(cubes, dtype=torch.int8, device=self.device)
        cube_mass = torch.empty(cubes, dtype=torch.float64, device=self.device)
        cube_open = torch.empty(cubes, dtype=torch.float64, device=self.device)
        cube_work = torch.empty(cubes, dtype=torch.int64, device=self.device)
        cube_leaves = torch.empty(cubes, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_mass_split_cubes(self._h, ptr(cube_off), ptr(cube_status), ptr(cube_mass), ptr(cube_open), ptr(cube_work),
                                               ptr(cube_leaves), _stream()))
        return (status, mass, true_mass, open_mass, work, leaves, depth_used, cube_off, cube_status, cube_mass, cube_open, cube_work,
                cube_leaves)

    def exact_models_at(self, ranks, rank_off, budget=0, stats=False):
        """The models of given ranks in exact_count's own order (pdp_exact_models_at): (status int8 [B]: 1 every rank of the instance is
        answered, -1 the budget ran out first, -2 more than 1023 variables, not searched; count_seen float64 [B]: the count when the search
        ended -- the model count if a rank >= it was asked; found int8 [K]: 1 the row is the model of that rank, 0 the instance has no
        model of that rank, -1 not known (budget, or status -2); models uint8 [sum K_b * n_b]: instance b's K_b rows of n_b bytes one after
        the other, instances in order, zero rows where found != 1; work int64 [B]), plus leaves int64 [B] with ``stats``.  ``rank_off``:
        int64 [B+1] on the problem's device, instance b asks for ranks[rank_off[b]:rank_off[b+1]]; ``ranks``: int64 [rank_off[B]] on the
        problem's device, non-decreasing inside an instance, each in 0 .. 2^53 - 1.  The model of a rank is a function of the instance
        and the rank alone.  ``budget`` as in exact_solve.  Synchronises the current stream, then asynchronous on it."""
        if isinstance(budget, bool) or not isinstance(budget, numbers.Integral):
            raise ValueError("budget must be an integer number of clause-literal reads (0: the library default), got %r" % (budget,))
        for name, t in (('rank_off', rank_off), ('ranks', ranks)):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != self.device:
                raise ValueError("%s must be an int64 tensor on %s, got %s" % (name, self.device, '%s on %s' % (t.dtype, t.device)
                                                                                if torch.is_tensor(t) else type(t).__name__))
        if rank_off.numel() != self.B + 1:
            raise ValueError("rank_off must have %d elements (one per instance and the end), got %d" % (self.B + 1, rank_off.numel()))
        rank_off, ranks = rank_off.reshape(-1).contiguous(), ranks.reshape(-1).contiguous()
        off = rank_off.cpu()
        K = int(off[-1])
        if ranks.numel() != K:
            raise ValueError("ranks must have rank_off[%d] = %d elements, got %d" % (self.B, K, ranks.numel()))
        nbytes = 0
        if K > 0 and self.R == 1 and int(off[0]) == 0 and bool((off[1:] >= off[:-1]).all()):
            # the rows' size; an unsound rank_off or a replicated problem goes to the library, which refuses before it writes anything
            if getattr(self, '_inst_n', None) is None:
                self._inst_n = torch.bincount(self.export_graph()[1].to(torch.int64), minlength=self.B).cpu()
            nbytes = int(((off[1:] - off[:-1]) * self._inst_n).sum())
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        count_seen = torch.empty(self.B, dtype=torch.float64, device=self.device)
        found = torch.empty(K, dtype=torch.int8, device=self.device)
        models = torch.empty(min(nbytes, 1 << 31), dtype=torch.uint8, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        leaves = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_models_at(self._h, ptr(rank_off), ptr(ranks), C.c_int64(int(budget)), ptr(status), ptr(count_seen), ptr(found),
                                        ptr(models), ptr(work), ptr(leaves), _stream()))
        return (status, count_seen, found, models, work, leaves) if stats else (status, count_seen, found, models, work)

    def exact_solve_assume(self, budget=0, hints=None, assume=None, arena=0, stats=False):
        """The learning search under assumptions (pdp_exact_solve_learn_assume): (status, model, work, failed), plus learned with
        ``stats``.  ``assume`` (int8, V elements, on the problem's device, or None): > 0 the variable is held true, < 0 held false, 0 free.
        status 1: model satisfies every clause and every assumption.  status 0: unsatisfiable under the assumptions, and failed int8 [V]
        is 1 on the assumed variables that are to blame (the instance plus those assumptions as unit clauses is unsatisfiable; none:
        the instance is unsatisfiable on its own) and 0 everywhere else.  An instance without an assumed variable gets exactly
        exact_solve(learn=True)'s outputs.  ``budget``, ``hints`` and ``arena`` as in exact_solve; exact_learn_reductions reports this
        call as well.  Asynchronous on the current stream."""
        if isinstance(arena, bool) or not isinstance(arena, numbers.Integral) or not 0 <= arena <= 1 << 30:
            raise ValueError("arena must be an integer from 0 to 2^30 words, got %r" % (arena,))
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable), got %s"
                                 % (self.V, '%s of %d' % (hints.dtype, hints.numel()) if torch.is_tensor(hints) else type(hints).__name__))
            hints = hints.reshape(-1).contiguous()
        if assume is not None:
            if not torch.is_tensor(assume) or assume.dtype != torch.int8 or assume.numel() != self.V or assume.device != self.device:
                raise ValueError("assume must be an int8 tensor of %d elements (one per variable) on %s, got %s"
                                 % (self.V, self.device, '%s of %d on %s' % (assume.dtype, assume.numel(), assume.device) if torch.is_tensor(assume)
                                    else type(assume).__name__))
            assume = assume.reshape(-1).contiguous()
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        learned = torch.empty(self.B, dtype=torch.int32, device=self.device)
        failed = torch.empty(self.V, dtype=torch.int8, device=self.device)
        check(lib().pdp_exact_solve_learn_assume(self._h, ptr(hints, torch.float32, self.V, 'hints'), ptr(assume, torch.int8, self.V, 'assume'),
                                                 C.c_int64(int(budget)), C.c_int64(int(arena)), ptr(status), ptr(model), ptr(work), ptr(learned),
                                                 ptr(failed), _stream()))
        return (status, model, work, failed, learned) if stats else (status, model, work, failed)

    def exact_learn_reductions(self):
        "int32 [B]: how often each instance's arena was reduced in the last exact_solve(learn=True) on this problem"
        out = torch.empty(self.B, dtype=torch.int32, device=self.device)
        check(lib().pdp_exact_learn_reductions(self._h, ptr(out), _stream()))
        return out

    def instance_edges(self):
        "int64 [B]: the literals (edges) of every instance"
        gm, _, bfm, _ = self.export_graph()
        return torch.bincount(bfm.long()[gm[1].long()], minlength=self.B)[:self.B]

    def _proof_regions(self, proof_off, proof=None):
        "proof_off as an int64 [B+1] tensor on the device, checked on the host (ascending from >= 0; ``proof`` holds the last offset)"
        if not torch.is_tensor(proof_off) or proof_off.dtype != torch.int64 or proof_off.numel() != self.B + 1:
            raise ValueError("proof_off must be an int64 tensor of %d elements (instances + 1), got %s"
                             % (self.B + 1, '%s of %d' % (proof_off.dtype, proof_off.numel()) if torch.is_tensor(proof_off) else type(proof_off).__name__))
        host = proof_off.detach().reshape(-1).cpu()
        if int(host[0]) < 0 or bool((host[1:] < host[:-1]).any()):
            raise ValueError("proof_off must ascend from an offset >= 0")
        if proof is not None:
            if not torch.is_tensor(proof) or proof.dtype != torch.int32 or proof.numel() < int(host[-1]):
                raise ValueError("proof must be an int32 tensor of at least proof_off[-1] = %d words, got %s"
                                 % (int(host[-1]), '%s of %d' % (proof.dtype, proof.numel()) if torch.is_tensor(proof) else type(proof).__name__))
        return proof_off.reshape(-1).contiguous().to(self.device), host

    def exact_solve_proof(self, budget=0, hints=None, arena=0, proof_off=None, proof=None):
        """The learning search (exact_solve(learn=True)) with its lemma log (pdp_exact_solve_learn_proof): (status, model, work, learned,
        proof int32, proof_off int64 [B+1], proof_len int64 [B]).  Every learned clause that is stored is appended to the instance's region
        proof[proof_off[b] : proof_off[b+1]] as ``len, lit_0 .. lit_{len-1}`` (literal (v << 1) | negative, v local to the instance) while
        whole lemmas fit; proof_len[b] is the number of words all of them need, so the proof of b is complete iff proof_len[b] <= its region.
        ``proof_off`` None: regions of PROOF_WORDS_PER_LITERAL words per literal of the instance.  ``proof``: a buffer to write into (the
        words outside the stored lemmas are not touched); None: a fresh zeroed one, or, with regions of no words at all, a sizing call that
        writes nothing and returns proof None."""
        if isinstance(arena, bool) or not isinstance(arena, numbers.Integral) or not 0 <= arena <= 1 << 30:
            raise ValueError("arena must be an integer from 0 to 2^30 words, got %r" % (arena,))
        if hints is not None:
            if not torch.is_tensor(hints) or hints.dtype != torch.float32 or hints.numel() != self.V:
                raise ValueError("hints must be a float32 tensor of %d elements (one per variable), got %s"
                                 % (self.V, '%s of %d' % (hints.dtype, hints.numel()) if torch.is_tensor(hints) else type(hints).__name__))
            hints = hints.reshape(-1).contiguous()
        if proof_off is None:
            e = self.instance_edges() if self.R == 1 else torch.zeros(self.B, dtype=torch.int64, device=self.device)   # R != 1: the library refuses
            proof_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(e * PROOF_WORDS_PER_LITERAL, 0)])
        proof_off, host = self._proof_regions(proof_off, proof)
        if proof is None and int(host[-1]) > int(host[0]):
            proof = torch.zeros(int(host[-1]), dtype=torch.int32, device=self.device)
        elif proof is not None:
            if not proof.is_cuda or not proof.is_contiguous():
                raise ValueError("proof must be a contiguous tensor on the problem's device")
        status = torch.empty(self.B, dtype=torch.int8, device=self.device)
        model = torch.empty(self.V, dtype=torch.float32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        learned = torch.empty(self.B, dtype=torch.int32, device=self.device)
        proof_len = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_solve_learn_proof(self._h, ptr(hints, torch.float32, self.V, 'hints'), C.c_int64(int(budget)), C.c_int64(int(arena)),
                                                ptr(status), ptr(model), ptr(work), ptr(learned), ptr(proof_off), ptr(proof), ptr(proof_len),
                                                _stream()))
        return status, model, work, learned, proof, proof_off, proof_len

    def exact_check(self, status, model, proof, proof_off, proof_len, budget=0):
        """Check the answers of a complete search (pdp_exact_check): (verdict int8 [B], fail_at int32 [B], work int64 [B]).  A status-1
        instance is checked against its model (verdict 0: fail_at = the lowest clause without a true literal); a status-0 instance against
        its proof, lemma by lemma and then the empty clause, each by unit propagation from the clauses and the lemmas before it (verdict 0:
        fail_at = the first lemma that does not follow, the number of lemmas for the empty clause).  Verdict -1: undecided status, incomplete
        proof (proof_len[b] past the region) or ``budget`` clause-literal reads spent.  ``proof`` None: every region must be empty."""
        for name, t, dt, k in (('status', status, torch.int8, self.B), ('model', model, torch.float32, self.V),
                               ('proof_len', proof_len, torch.int64, self.B)):
            if not torch.is_tensor(t) or t.dtype != dt or t.numel() != k:
                raise ValueError("%s must be a %s tensor of %d elements, got %s"
                                 % (name, dt, k, '%s of %d' % (t.dtype, t.numel()) if torch.is_tensor(t) else type(t).__name__))
        proof_off, host = self._proof_regions(proof_off, proof)
        if proof is None and int(host[-1]) > int(host[0]):
            raise ValueError("proof is None but the regions hold %d words" % (int(host[-1]) - int(host[0])))
        if proof is not None and (not proof.is_cuda or not proof.is_contiguous()):
            raise ValueError("proof must be a contiguous tensor on the problem's device")
        verdict = torch.empty(self.B, dtype=torch.int8, device=self.device)
        fail_at = torch.empty(self.B, dtype=torch.int32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        check(lib().pdp_exact_check(self._h, ptr(status.reshape(-1).contiguous()), ptr(model.reshape(-1).contiguous()), ptr(proof_off), ptr(proof),
                                    ptr(proof_len.reshape(-1).contiguous()), C.c_int64(int(budget)), ptr(verdict), ptr(fail_at), ptr(work), _stream()))
        return verdict, fail_at, work

    def exact_trim(self, status, proof, proof_off, proof_len, budget=0, keep=None):
        """The backward check of the proofs of the status-0 instances (pdp_exact_trim): (verdict int8 [B], fail_at int32 [B], work int64 [B],
        core int8 [F], keep int8 of proof's size, n_core int32 [B], n_keep int32 [B]).  From the empty clause backwards only the lemmas that
        are needed are checked, each by unit propagation from the clauses and the lemmas before it.  Verdict 1: core[c] = 1 on the original
        clauses the refutation rests on (they are unsatisfiable on their own) and keep = 1 on every word of a needed lemma (the kept lemmas
        are a proof against the core alone; exact.trimmed compacts them).  Verdict 0: fail_at = the first malformed lemma, else the needed
        lemma that does not follow; verdict -1: a status other than 0, an incomplete proof (proof_len[b] past the region) or ``budget``
        clause-literal reads spent; core and keep are then 0.  keep is allocated at proof's size (``keep``: an int8 buffer of that size to
        write into instead); its words past proof_len[b] in a region, and the regions of instances that are not judged, are not written:
        0 in the buffer allocated here, whatever they held in a buffer that was passed in.  ``proof`` None: every region must be empty, keep is None."""
        for name, t, dt, k in (('status', status, torch.int8, self.B), ('proof_len', proof_len, torch.int64, self.B)):
            if not torch.is_tensor(t) or t.dtype != dt or t.numel() != k:
                raise ValueError("%s must be a %s tensor of %d elements, got %s"
                                 % (name, dt, k, '%s of %d' % (t.dtype, t.numel()) if torch.is_tensor(t) else type(t).__name__))
        proof_off, host = self._proof_regions(proof_off, proof)
        if proof is None and int(host[-1]) > int(host[0]):
            raise ValueError("proof is None but the regions hold %d words" % (int(host[-1]) - int(host[0])))
        if proof is not None and (not proof.is_cuda or not proof.is_contiguous()):
            raise ValueError("proof must be a contiguous tensor on the problem's device")
        verdict = torch.empty(self.B, dtype=torch.int8, device=self.device)
        fail_at = torch.empty(self.B, dtype=torch.int32, device=self.device)
        work = torch.empty(self.B, dtype=torch.int64, device=self.device)
        core = torch.empty(self.F, dtype=torch.int8, device=self.device)
        if keep is not None and (proof is None or not torch.is_tensor(keep) or keep.dtype != torch.int8 or keep.numel() != proof.numel()
                                 or not keep.is_cuda or not keep.is_contiguous()):
            raise ValueError("keep must be a contiguous int8 tensor of proof's size on the problem's device")
        if keep is None and proof is not None:
            keep = torch.zeros(proof.numel(), dtype=torch.int8, device=self.device)
        n_core = torch.empty(self.B, dtype=torch.int32, device=self.device)
        n_keep = torch.empty(self.B, dtype=torch.int32, device=self.device)
        check(lib().pdp_exact_trim(self._h, ptr(status.reshape(-1).contiguous().to(self.device)), ptr(proof_off), ptr(proof),
                                   ptr(proof_len.reshape(-1).contiguous().to(self.device)), C.c_int64(int(budget)), ptr(verdict), ptr(fail_at),
                                   ptr(work), ptr(core), ptr(keep), ptr(n_core), ptr(n_keep), _stream()))
        return verdict, fail_at, work, core, keep, n_core, n_keep

    def exact_last_grid(self):
        """Workgroups of the last launch of exact_solve, exact_solve_split, exact_count_split, exact_min_unsat_split, exact_nearest_split, exact_mass_split, exact_count_round, exact_solve_round and exact_nearest_round (their cube kernels), exact_min_unsat, exact_nearest, exact_count, exact_mass, exact_models_at, exact_solve_proof, exact_check or exact_trim on this problem (pdp_exact_last_grid), 0 before the
        first; PDP_EXACT_GRID=<v> in the environment lowers a launch to min(grid, v).  A host read: it does not synchronise."""
        out = C.c_int32(-1)
        check(lib().pdp_exact_last_grid(self._h, C.byref(out)))
        return int(out.value)

    # -- K14 ---------------------------------------------------------------------------------------------------
    def energy(self, assignment):
        en = torch.empty(self.B, 1, dtype=torch.float32, device=self.device)
        uf = torch.empty(self.F, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_energy(self._h, ptr(assignment, torch.float32, self.V), ptr(en), ptr(uf), _stream()))
        return en, uf

    def energy_diff(self, assignment):
        d = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_energy_diff(self._h, ptr(assignment, torch.float32, self.V), ptr(d), _stream()))
        return d

    def set_rng_base(self, first_variable, first_instance):
        """this batch is a contiguous part of a larger forward: the Philox draws are counted from there (include/pdp_hip.h)"""
        check(lib().pdp_problem_set_rng_base(self._h, C.c_uint32(int(first_variable)), C.c_uint32(int(first_instance))))

    def set_exchange(self, fn):
        """``fn(mins, maxs, ors)``: three numpy uint32 arrays to be replaced, in place, by their element-wise minimum / maximum / bit-wise OR
        over all parts of a coupled forward solved by several processes (include/pdp_hip.h: pdp_problem_set_exchange); None removes it."""
        if fn is None:
            self._exchange_cb = None
            check(lib().pdp_problem_set_exchange(self._h, None, None))
            return
        import numpy as np

        def trampoline(user, mins, n_mins, maxs, n_maxs, ors, n_ors):
            try:
                view = lambda ptr, n: np.ctypeslib.as_array(ptr, shape=(n,)) if n > 0 else np.zeros(0, np.uint32)
                fn(view(mins, n_mins), view(maxs, n_maxs), view(ors, n_ors))
                return 0
            except Exception:                      # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1

        self._exchange_cb = EXCHANGE_FN(trampoline)          # (kept alive as long as the problem uses it)
        check(lib().pdp_problem_set_exchange(self._h, self._exchange_cb, None))

    def random_fill(self, values=None, seed=0):
        mode = RNG_STREAM if values is not None else RNG_PHILOX
        check(lib().pdp_random_fill(self._h, C.c_int(mode), ptr(values, torch.float32), C.c_uint64(seed), _stream()))

    def local_search(self, pred, iterations, epsilon, var_rand=None, coin_rand=None, seed=0):
        out = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        steps = C.c_int32(0)
        mode = RNG_STREAM if var_rand is not None else RNG_PHILOX
        check(lib().pdp_local_search(self._h, ptr(pred, torch.float32, self.V, 'prediction'), C.c_int(iterations), C.c_float(epsilon),
                                     C.c_int(mode), ptr(var_rand, torch.float32), ptr(coin_rand, torch.float32),
                                     C.c_uint64(seed), ptr(out), C.byref(steps), _stream()))
        return out, int(steps.value)

    def deduplicate(self, pred):
        out = torch.empty(self.V // self.R, 1, dtype=torch.float32, device=self.device)
        chosen = torch.empty(self.B // self.R, dtype=torch.int32, device=self.device)
        check(lib().pdp_deduplicate(self._h, ptr(pred, torch.float32, self.V), ptr(out), ptr(chosen), _stream()))
        return out, chosen

    # -- neural plug-ins -------------------------------------------------------------------------------------------------
    def neural_aggregate_edges(self, agg_w, by_variable, state, edge_mask, active_mask, old, out=None):
        if out is None:
            out = torch.empty(self.E, agg_w.desc.out, dtype=torch.float32, device=self.device)
        check(lib().pdp_neural_aggregate_edges(self._h, C.byref(agg_w.desc), C.c_int(1 if by_variable else 0),
                                               ptr(state, torch.float32, self.E * (agg_w.desc.din - 1), 'state'),
                                               ptr(edge_mask, torch.float32, self.E, 'edge_mask'), ptr(active_mask, torch.uint8, self.B, 'active_mask'),
                                               ptr(old, torch.float32, self.E * agg_w.desc.out, 'init_state'),
                                               ptr(out, torch.float32, self.E * agg_w.desc.out, 'out'), _stream()))
        return out

    def neural_gru(self, gru_w, state, h, active_mask, out=None):
        if out is None:
            out = torch.empty(self.E, gru_w.desc.H, dtype=torch.float32, device=self.device)
        check(lib().pdp_neural_gru(self._h, C.byref(gru_w.desc), ptr(state, torch.float32, self.E * gru_w.desc.dx, 'message_state'),
                                   ptr(h, torch.float32, self.E * gru_w.desc.H, 'init_state'), ptr(active_mask, torch.uint8, self.B, 'active_mask'),
                                   ptr(out, torch.float32, self.E * gru_w.desc.H, 'out'), _stream()))
        return out

    def neural_predict(self, agg_w, head_w, state, edge_mask):
        out = torch.empty(self.V, 1, dtype=torch.float32, device=self.device)
        check(lib().pdp_neural_predict(self._h, C.byref(agg_w.desc), C.byref(head_w.desc), ptr(state, torch.float32, self.E * (agg_w.desc.din - 1), 'state'),
                                       ptr(edge_mask, torch.float32, self.E, 'edge_mask'), ptr(out), _stream()))
        return out

    # -- persistent solve -----------------------------------------------------------------------------------------
    def sp_solve(self, q, fs, active_mask, dec, iterations, tolerance, t_max, pi=0.0, model=MODEL_SP,
                 decimation_probability=0.5, seed=0, coins=None, check_termination=True, time_kernels=False, replicas_identical=False, isolate_instances=False,
                 inputs_disposable=False):
        a = SolveArgs()
        a.inputs_disposable = 1 if inputs_disposable else 0
        a.isolate_instances = 1 if isolate_instances else 0
        a.time_kernels = 1 if time_kernels else 0
        a.replicas_identical = 1 if replicas_identical else 0
        a.model = model; a.iterations = iterations; a.tolerance = tolerance; a.t_max = t_max; a.pi = pi
        a.decimation_probability = decimation_probability; a.seed = seed
        a.coins = ptr(coins, torch.float32).value if coins is not None else None
        a.q = ptr(q, torch.float32, 3 * self.E).value; a.fs = ptr(fs, torch.float32, 2 * self.E).value
        a.active_mask = ptr(active_mask, torch.uint8, self.B).value
        a.decimator = dec._h.value
        a.check_termination = 1 if check_termination else 0
        check(lib().pdp_sp_solve(self._h, C.byref(a), _stream()))
        self.last_solve_launches = int(a.kernel_launches_host)
        self.last_solve_stats = dict(launches=int(a.kernel_launches_host), replays=int(a.replay_launches_host),
                                     solve_kernel_ms=float(a.solve_kernel_ms_host), replay_kernel_ms=float(a.replay_kernel_ms_host),
                                     hbm_instances=int(a.hbm_instances_host))
        return int(a.iterations_run_host), bool(a.used_lds_host)


# -- the reference's L0 primitives on a sparse COO mask (include/pdp_hip.h: pdp_coo_*, pdp_csr_*) -------------------------------------------
def coo_reduce(kind, rows, cols, x, n_rows, n_cols):
    "util.sparse_max ('max') / sparse_argmax ('argmax') of x [nnz] paired with the entries (rows[i], cols[i]) of a [n_rows, n_cols] mask"
    require_gpu()
    nnz = int(rows.numel())
    scratch = torch.empty(n_cols + 2, dtype=torch.int64, device=x.device)
    out = torch.empty(n_cols, dtype=torch.float32 if kind == 'max' else torch.int64, device=x.device)
    fn = lib().pdp_coo_max if kind == 'max' else lib().pdp_coo_argmax
    check(fn(ptr(rows, torch.int64, nnz, 'mask rows'), ptr(cols, torch.int64, nnz, 'mask columns'), C.c_int64(nnz), ptr(x, torch.float32, nnz, 'x'),
             C.c_int64(n_rows), C.c_int64(n_cols), ptr(scratch), ptr(out), _stream()))
    return out


class CsrMask(object):
    "row offsets / columns / values of the row-sorted entries of a sparse mask [n_rows, n_cols] (built once per mask, cached on the tensor)"

    def __init__(self, mask):
        require_gpu()
        m = mask if mask.is_coalesced() else mask.coalesce()
        idx = m.indices()
        self.n_rows, self.n_cols = int(mask.size(0)), int(mask.size(1))
        self.rows = idx[0].contiguous()
        self.cols = idx[1].contiguous()
        self.vals = m.values().to(torch.float32).contiguous()
        self.nnz = int(self.cols.numel())
        self.row_ptr = torch.empty(self.n_rows + 1, dtype=torch.int64, device=mask.device)
        check(lib().pdp_coo_row_ptr(ptr(self.rows, torch.int64), C.c_int64(self.nnz), C.c_int64(self.n_rows), ptr(self.row_ptr), _stream()))

    def matmul(self, X, sub=None):
        "mask @ X (- sub): X [n_cols, d] dense"
        d = int(X.size(1))
        if X.size(0) != self.n_cols:
            raise NativeError("mask [%d, %d] times a matrix with %d rows" % (self.n_rows, self.n_cols, X.size(0)))
        out = torch.empty(self.n_rows, d, dtype=torch.float32, device=X.device)
        check(lib().pdp_csr_matmul(ptr(self.row_ptr), ptr(self.cols), ptr(self.vals), C.c_int64(self.n_rows), ptr(X, torch.float32, self.n_cols * d, 'X'),
                                   C.c_int(d), C.c_int64(d), ptr(sub, torch.float32, self.n_rows * d, 'sub') if sub is not None else None, ptr(out), _stream()))
        return out

    def smooth_max(self, x, alpha):
        out = torch.empty(self.n_rows, 1, dtype=torch.float32, device=x.device)
        check(lib().pdp_csr_smooth_max(ptr(self.row_ptr), ptr(self.cols), ptr(self.vals), C.c_int64(self.n_rows), ptr(x, torch.float32, self.n_cols, 'x'),
                                       C.c_float(alpha), ptr(out), _stream()))
        return out


def dimacs_parse(path):
    """One DIMACS file -> (var_num, clause_num, signed_vars int32 [E], clause_ids int32 [E]) in the compact conventions of the
    reference's converter (include/pdp_hip.h, pdp_dimacs_open).  Host code only: works without a GPU."""
    import numpy as np
    h = C.c_void_p()
    nv, nc, ne = C.c_int32(), C.c_int32(), C.c_int64()
    check(lib().pdp_dimacs_open(os.fsencode(path), C.byref(h), C.byref(nv), C.byref(nc), C.byref(ne)))
    try:
        sv = np.empty(ne.value, np.int32); ci = np.empty(ne.value, np.int32)
        check(lib().pdp_dimacs_read(h, sv.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p)))
    finally:
        lib().pdp_dimacs_close(h)
    return int(nv.value), int(nc.value), sv, ci


def dimacs_parse_many(paths, threads=8):
    """Several DIMACS files at once (parsed by host threads inside the library): list of dimacs_parse tuples in input order."""
    import numpy as np
    n = len(paths)
    if n == 0:
        return []
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    handles = (C.c_void_p * n)()
    nv = (C.c_int32 * n)(); nc = (C.c_int32 * n)(); ne = (C.c_int64 * n)()
    check(lib().pdp_dimacs_open_many(arr, C.c_int32(n), C.c_int32(threads), handles, nv, nc, ne))
    out = []
    try:
        for i in range(n):
            sv = np.empty(ne[i], np.int32); ci = np.empty(ne[i], np.int32)
            check(lib().pdp_dimacs_read(C.c_void_p(handles[i]), sv.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p)))
            out.append((int(nv[i]), int(nc[i]), sv, ci))
    finally:
        for i in range(n):
            if handles[i]:
                lib().pdp_dimacs_close(C.c_void_p(handles[i]))
    return out


TIMING_KEYS = ('agg_pre', 'row_sum', 'agg_post', 'gru', 'predict_head', 'walksat', 'sp_adaptors', 'sp_sweep')       # include/pdp_hip.h: PDP_TK_*


def kernel_timing(enable):
    "bracket the library's neural / Walk-SAT kernels with HIP events on their launch stream (measurement only)"
    global _TIMING_ON
    check(lib().pdp_kernel_timing(C.c_int(1 if enable else 0)))
    _TIMING_ON = bool(enable)


_TIMING_ON = False


def kernel_timing_enabled():
    "event pairs around every launch cannot be read back from a replayed graph: the solver's graph loop stands back while this is on"
    return _TIMING_ON


def kernel_timing_read():
    "{key: (summed device ms, launches)} since the last read; synchronises on the recorded events"
    ms = (C.c_float * len(TIMING_KEYS))(); n = (C.c_int32 * len(TIMING_KEYS))()
    check(lib().pdp_kernel_timing_read(ms, n))
    return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(TIMING_KEYS)}


NAME_KEYS = TIMING_KEYS + ('sp_solve', 'sp_replay')                                         # include/pdp_hip.h: PDP_KN_*


def kernel_name(key):
    "name, with template arguments, of the kernel the library launched last for this key ('' before the first launch)"
    buf = C.create_string_buffer(160)
    check(lib().pdp_kernel_name(C.c_int(NAME_KEYS.index(key)), buf, C.c_int(160)))
    return buf.value.decode('ascii')


def math_apply(fn, x):
    names = {'exp': 0, 'log': 1, 'logsigmoid': 2, 'sigmoid': 3, 'tanh': 4, 'safe_exp': 5, 'safe_log': 6, 'philox': 7, 'rcp': 8, 'safe_exp_fast': 9, 'safe_log_fin': 10, 'safe_log_fin_scorer': 11, 'exp_fin': 12, 'tanh_abs': 13, 'rcp_ge1': 14}
    require_gpu()
    y = torch.empty_like(x)
    check(lib().pdp_math_apply(C.c_int(names[fn]), ptr(x, torch.float32), ptr(y), C.c_int64(x.numel()), _stream()))
    return y
