"""Shared pieces of the exhaustive sweeps of include/pdp_math.h (tests/test_math_sweep_host.py, tests/test_math_sweep_gpu.py,
tools/math_checksums.py).  No tests here.

A single-argument fp32 function has 2^32 inputs.  The oracle (the CPU build of the header) is run over all of them once by
tools/math_checksums.py, which records three sums per block of BLOCK inputs in tests/golden/math_checksums.npz; the GPU test recomputes
the sums of every block on the device and compares.  The accuracy statements are written once, on integer keys of the bit patterns, so
that numpy (the oracle, on the CPU) and torch (the kernels, on the device) evaluate the very same conditions.
"""
import os
import zipfile

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'math_checksums.npz')

# every single-argument probe of native.math_apply / oracle.math_apply.  Not here: 'philox' (a function of the index, not of x) and
# 'rcp_ge1', whose device and host forms agree on [1, 2^126] only (outside it the Newton steps and the IEEE division part ways by
# design) and which tests/test_hip_ops.py::test_reciprocal_exhaustive already sweeps over exactly that range.
PROBES = ('exp', 'log', 'logsigmoid', 'sigmoid', 'tanh', 'tanh_abs', 'safe_exp', 'safe_log', 'rcp', 'safe_exp_fast', 'safe_log_fin',
          'safe_log_fin_scorer', 'exp_fin')
ACCURACY_FUNCTIONS = ('exp', 'log', 'logsigmoid', 'sigmoid', 'tanh', 'tanh_abs')

BLOCK = 1 << 22                          # sums stay below 2^16 * 2^22 * 2^22 = 2^60: no wrap-around in int64 or uint64
N_BLOCKS = (1 << 32) // BLOCK
NAN_BITS = 0x7fc00000
INF_BITS = 0x7f800000


def blocks():
    "(index, first bit pattern) of every aligned block of BLOCK inputs, 0 .. 2^32 - 1"
    for k in range(N_BLOCKS):
        yield k, k * BLOCK


def block_of(bits):
    return int(bits) // BLOCK


def fbits(v):
    "bit pattern of float32(v)"
    return int(np.asarray(v, dtype=np.float32).reshape(1).view(np.uint32)[0])


def key_of(bits):
    "sign-magnitude key of a bit pattern: ordered like the floats (both zeros -> 0); |key| > INF_BITS means NaN"
    bits = int(bits)
    return bits if bits < (1 << 31) else -(bits - (1 << 31))


def K(v):
    return key_of(fbits(v))


# ---- the two array back ends ---------------------------------------------------------------------------------------------------
class NumpyOps(object):
    name = 'numpy'

    def input_bits(self, start, n):
        return np.arange(start, start + n, dtype=np.int64)

    def as_float(self, bits):
        return bits.astype(np.uint32).view(np.float32)

    def out_bits(self, y):
        "bit patterns as int64 in [0, 2^32), every NaN as NAN_BITS"
        b = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32)
        return np.where((b & np.uint32(0x7fffffff)) > np.uint32(INF_BITS), np.uint32(NAN_BITS), b).astype(np.int64)

    def weighted_sums(self, a, w):
        return a @ w                                          # integer product, no temporary

    def weights(self):
        return np.arange(1, BLOCK + 1, dtype=np.int64)

    def f64(self, a):
        return a.astype(np.float64)

    def f32(self, a):
        return a.astype(np.float32)

    def spacing(self, a32):
        "distance from |a32| to the next float32 above it, as float64"
        a = np.abs(a32)
        with np.errstate(over='ignore', invalid='ignore'):
            return np.nextafter(a, np.float32(np.inf)).astype(np.float64) - a.astype(np.float64)

    def min0(self, x):
        return np.minimum(x, 0.0)

    def max_const(self, x, c):
        return np.maximum(x, np.float32(c))

    def floor_at(self, a, lo):
        return np.maximum(a, lo)

    where, abs, exp, log, log1p, tanh = (staticmethod(f) for f in (np.where, np.abs, np.exp, np.log, np.log1p, np.tanh))

    def zeros_like(self, a):
        return np.zeros_like(a)

    def max_at(self, a):
        i = int(np.argmax(a))
        return float(a[i]), i

    def count_first(self, bad):
        n = int(np.count_nonzero(bad))
        return n, (int(np.argmax(bad)) if n else -1)

    def item(self, a, i):
        return a[i].item()

    def quiet(self):
        return np.errstate(all='ignore')


class TorchOps(object):
    name = 'torch'

    def __init__(self, device):
        import torch
        self.t = torch
        self.device = device
        self.where, self.abs, self.exp, self.log, self.log1p, self.tanh = torch.where, torch.abs, torch.exp, torch.log, torch.log1p, torch.tanh

    def input_bits(self, start, n):
        return self.t.arange(start, start + n, dtype=self.t.int64, device=self.device)

    def as_float(self, bits):
        return (bits - ((bits >> 31) << 32)).to(self.t.int32).view(self.t.float32)       # 2^31 .. 2^32 - 1 -> the negative int32 of the same bits

    def out_bits(self, y):
        b = y.contiguous().view(self.t.int32).to(self.t.int64) & 0xffffffff
        return self.t.where((b & 0x7fffffff) > INF_BITS, self.t.full_like(b, NAN_BITS), b)

    def weights(self):
        return self.t.arange(1, BLOCK + 1, dtype=self.t.int64, device=self.device)

    def weighted_sums(self, a, w):
        return (a * w).sum(1)

    def f64(self, a):
        return a.to(self.t.float64)

    def f32(self, a):
        return a.to(self.t.float32)

    def spacing(self, a32):
        a = a32.abs()
        return self.t.nextafter(a, a.new_tensor(float('inf'))).to(self.t.float64) - a.to(self.t.float64)

    def min0(self, x):
        return self.t.clamp(x, max=0.0)

    def max_const(self, x, c):
        return self.t.maximum(x, x.new_tensor(float(np.float32(c))))

    def floor_at(self, a, lo):
        return self.t.clamp(a, min=lo)

    def zeros_like(self, a):
        return self.t.zeros_like(a)

    def max_at(self, a):
        i = int(self.t.argmax(a).item())
        return float(a[i].item()), i

    def count_first(self, bad):
        n = int(bad.sum().item())
        return n, (int(self.t.argmax(bad.to(self.t.uint8)).item()) if n else -1)

    def item(self, a, i):
        return a[i].item()

    def quiet(self):
        import contextlib
        return contextlib.nullcontext()


# ---- checksum --------------------------------------------------------------------------------------------------------------------
def checksum(ops, y, weights=None):
    """[n_blocks, 3] int64 sums of the outputs y of a whole number of consecutive blocks: with b_i the output's bit pattern (NaNs
    canonical, the sign of a zero kept) and w_i = index inside the block + 1: sum b_i, sum (b_i & 0xffff) w_i, sum (b_i >> 16) w_i."""
    w = ops.weights() if weights is None else weights
    b = ops.out_bits(y).reshape(-1, BLOCK)
    s0 = b.sum(1)
    s1 = ops.weighted_sums(b & 0xffff, w)
    s2 = ops.weighted_sums(b >> 16, w)
    if ops.name == 'numpy':
        return np.stack([s0, s1, s2], axis=1)
    return ops.t.stack([s0, s1, s2], dim=1)


def load_fixture():
    "uint64 [len(PROBES), N_BLOCKS, 3] of the recorded oracle, after checking that the file was made for these probes and this BLOCK"
    with np.load(GOLDEN_FILE) as z:
        assert int(z['block']) == BLOCK and tuple(str(s) for s in z['probes']) == PROBES, "regenerate with tools/math_checksums.py"
        sums = z['sums']
    assert sums.dtype == np.uint64 and sums.shape == (len(PROBES), N_BLOCKS, 3)
    return sums


def save_fixture(path, sums):
    "an .npz whose bytes depend on its contents only (np.savez stamps the time of day into the archive)"
    assert sums.dtype == np.uint64 and sums.shape == (len(PROBES), N_BLOCKS, 3)
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as z:
        for name, arr in (('sums', sums), ('probes', np.array(PROBES)), ('block', np.array(BLOCK, dtype=np.int64))):
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asarray(arr), allow_pickle=False)


# ---- accuracy against float64 ----------------------------------------------------------------------------------------------------
def ulp_err(got, want64):
    "numpy: |got - want64| in units of the spacing of float32(want64), floored at 2^-149 (tests/test_fast_build_gpu.py::_ulp_err)"
    return _ulp_err(NumpyOps(), got, want64)


def ulp_err_torch(got, want64):
    "the same on torch tensors, the spacing from torch.nextafter"
    return _ulp_err(TorchOps(got.device), got, want64)


def _ulp_err(ops, got, want64):
    with ops.quiet():
        ulp = ops.floor_at(ops.spacing(ops.f32(want64)), 2.0 ** -149)
        return ops.abs(ops.f64(got) - want64) / ulp


def reference64(ops, fn, x64):
    "float64 value of the function that probe `fn` approximates"
    with ops.quiet():
        if fn == 'exp':
            return ops.exp(x64)
        if fn == 'log':
            return ops.log(x64)
        if fn == 'logsigmoid':
            return ops.min0(x64) - ops.log1p(ops.exp(-ops.abs(x64)))
        if fn == 'sigmoid':
            return 1.0 / (1.0 + ops.exp(-x64))
        if fn in ('tanh', 'tanh_abs'):
            return ops.tanh(x64)
    raise KeyError(fn)


# What tools/math_checksums.py --accuracy measured for the oracle over the whole domain of each statement: (worst input, error).  The
# device's bits are the oracle's, so the GPU sweep must find the same figures; tests/test_math_sweep_host.py re-evaluates each worst
# input with the live oracle.  The relative bounds of sigmoid and tanh, for which the project stated no figure, are these maxima
# rounded up to the next half ulp.
ORACLE_WORST = {                                       # (function, kind, statement) -> (input bits, error)
    ('exp', 'ulp', 'x in [-104, 88.72]'): (0xc0bc17a1, 1.0103),
    ('log', 'ulp', 'x > 0 finite'): (0x3fb4f239, 0.8265),
    ('logsigmoid', 'ulp', 'x finite'): (0x405cd015, 2.9313),
    ('sigmoid', 'ulp', 'x in [-87, FLT_MAX]'): (0xc18515ec, 2.4807),
    ('sigmoid', 'abs', 'x finite'): (0x40fb7ea8, 8.9307e-08),
    ('tanh', 'ulp', 'x finite'): (0x3e339d62, 2.8284),
    ('tanh', 'abs', 'x finite'): (0x405dc73d, 8.9294e-08),
    ('tanh_abs', 'abs', 'x finite'): (0x3934e004, 1.1915e-07),
}


def same_input(fn, a, b):
    "the tanh forms are odd, bit for bit, and so is their error: x and -x tie"
    return (a ^ b) & (0x7fffffff if fn in ('tanh', 'tanh_abs') else 0xffffffff) == 0


def same_figure(measured, recorded):
    "a recorded figure has five digits; two float64 libraries differ far below that"
    return abs(measured - recorded) <= 2e-4 * recorded

FINITE = lambda k: (k > -INF_BITS) & (k < INF_BITS)            # noqa: E731
IS_NAN = lambda k: (k > INF_BITS) | (k < -INF_BITS)            # noqa: E731


def statements(fn, apply_one):
    """The accuracy statements about probe `fn`, as (kind, name, domain, arg) over arrays k (input keys), b (output bits) and y (outputs):
    ('ulp' | 'abs', name, domain(k), bound): the largest error over the domain stays within the bound;
    ('all', name, domain(k), holds(k, b, y)): holds for every input of the domain.
    apply_one(fn, value) evaluates the function under test at one float and returns the output's bit pattern."""
    nan_in_nan_out = ('all', 'NaN -> NaN', IS_NAN, lambda k, b, y: b == NAN_BITS)
    within_one = lambda k, b, y: (b & 0x7fffffff) <= 0x3f800000                                     # noqa: E731
    if fn == 'exp':
        lo, hi, ovf = K(-104.0), K(88.72), K(88.7229)
        return [('ulp', 'x in [-104, 88.72]', lambda k: (k >= lo) & (k <= hi), 1.5),
                ('all', 'x >= 88.7229 -> +inf', lambda k: (k >= ovf) & (k <= INF_BITS), lambda k, b, y: b == INF_BITS),
                ('all', 'x < -104 -> +0', lambda k: (k < lo) & (k >= -INF_BITS), lambda k, b, y: b == 0),
                nan_in_nan_out]
    if fn == 'log':
        one = K(1.0)
        return [('ulp', 'x > 0 finite', lambda k: (k > 0) & (k < INF_BITS), 1.5),
                ('all', 'log(1) == 0', lambda k: k == one, lambda k, b, y: (b & 0x7fffffff) == 0),
                ('all', '+-0 -> -inf', lambda k: k == 0, lambda k, b, y: b == 0xff800000),
                ('all', 'x < 0 -> NaN', lambda k: (k < 0) & (k >= -INF_BITS), lambda k, b, y: b == NAN_BITS),
                ('all', '+inf -> +inf', lambda k: k == INF_BITS, lambda k, b, y: b == INF_BITS),
                nan_in_nan_out]
    if fn == 'logsigmoid':
        return [('ulp', 'x finite', FINITE, 3.0), nan_in_nan_out]
    if fn == 'tanh_abs':
        return [('abs', 'x finite', FINITE, 1.2e-7), ('all', '|y| <= 1', FINITE, within_one), nan_in_nan_out]
    if fn == 'sigmoid':
        m87 = K(-87.0)
        floor = apply_one('sigmoid', -87.0)
        return [('abs', 'x finite', FINITE, 1.5e-7),
                ('all', 'y in [0, 1]', FINITE, lambda k, b, y: b <= 0x3f800000),
                ('all', 'x < -87 -> sigmoid(-87)', lambda k: (k < m87) & (k > -INF_BITS), lambda k, b, y: b == floor),
                ('ulp', 'x in [-87, FLT_MAX]', lambda k: (k >= m87) & (k < INF_BITS), 2.5),
                nan_in_nan_out]
    if fn == 'tanh':
        return [('abs', 'x finite', FINITE, 2e-7), ('all', '|y| <= 1', FINITE, within_one), ('ulp', 'x finite', FINITE, 3.0), nan_in_nan_out]
    raise KeyError(fn)


# The lean and select-free forms against the general ones (include/pdp_math.h: "same results as the general functions on their stated
# domain"): (lean probe, general probe, clamp applied to x before the general probe or None, domain(k)).  Bit for bit, NaN == NaN.
SCORER_EPS = 1e-10
LEAN_FORMS = [
    ('safe_exp_fast', 'safe_exp', None, lambda k: k == k),
    ('exp_fin', 'safe_exp', None, lambda k: ((k > -INF_BITS) & (k <= K(30.0))) | IS_NAN(k)),
    ('exp', 'safe_exp', None, lambda k: (k >= -INF_BITS) & (k <= K(30.0))),
    ('safe_log_fin', 'safe_log', None, lambda k: FINITE(k) | IS_NAN(k)),
    ('safe_log_fin_scorer', 'log', SCORER_EPS, lambda k: FINITE(k) | IS_NAN(k)),
]


def keys(ops, start, n):
    xb = ops.input_bits(start, n)
    return xb, ops.where(xb < (1 << 31), xb, (1 << 31) - xb)


def lean_mismatches(ops, apply, relation, start, n):
    "(count, first input bits, lean output bits, general output bits) over the inputs start .. start + n - 1 that lie in the domain"
    lean, general, eps, domain = relation
    xb, k = keys(ops, start, n)
    x = ops.as_float(xb)
    a = ops.out_bits(apply(lean, x))
    g = ops.out_bits(apply(general, x if eps is None else ops.max_const(x, eps)))
    cnt, i = ops.count_first(domain(k) & (a != g))
    return (cnt, start + i, int(ops.item(a, i)), int(ops.item(g, i))) if cnt else (0, -1, 0, 0)


def odd_mismatches(ops, apply, fn, start, n):
    "the same for bits(f(-x)) == bits(f(x)) ^ 0x80000000 over the non-NaN x >= 0 with bit patterns start .. start + n - 1 (< 2^31)"
    xb, k = keys(ops, start, n)
    p = ops.out_bits(apply(fn, ops.as_float(xb)))
    m = ops.out_bits(apply(fn, ops.as_float(xb + (1 << 31))))
    ok = (m == (p ^ (1 << 31))) | ((p == NAN_BITS) & (m == NAN_BITS))
    cnt, i = ops.count_first((k <= INF_BITS) & ~ok)
    return (cnt, start + i, int(ops.item(p, i)), int(ops.item(m, i))) if cnt else (0, -1, 0, 0)


class Tally(object):
    "what the statements of one function amount to over the chunks seen so far"

    def __init__(self, fn, apply_one):
        self.fn = fn
        self.stmts = statements(fn, apply_one)
        self.worst = {}                                      # (kind, name) -> (error, input bits, output bits)
        self.broken = {}                                     # name -> (count, first input bits, its output bits)
        self.seen = 0

    def add(self, ops, start, y):
        "y = outputs of the inputs with bit patterns start .. start + len(y) - 1"
        n = int(y.shape[0])
        xb = ops.input_bits(start, n)
        k = ops.where(xb < (1 << 31), xb, (1 << 31) - xb)
        b = ops.out_bits(y)
        err = {}
        if any(s[0] in ('ulp', 'abs') for s in self.stmts):
            with ops.quiet():
                want = reference64(ops, self.fn, ops.f64(ops.as_float(xb)))
                if any(s[0] == 'ulp' for s in self.stmts):
                    err['ulp'] = _ulp_err(ops, y, want)
                if any(s[0] == 'abs' for s in self.stmts):
                    err['abs'] = ops.abs(ops.f64(y) - want)
        for kind, name, domain, arg in self.stmts:
            dom = domain(k)
            if kind == 'all':
                cnt, i = ops.count_first(dom & ~arg(k, b, y))
                if cnt:
                    c0, x0, y0 = self.broken.get(name, (0, start + i, int(ops.item(b, i))))
                    self.broken[name] = (c0 + cnt, x0, y0)
            else:
                e, i = ops.max_at(ops.where(dom, err[kind], ops.zeros_like(err[kind])))
                if e != e:
                    e = float('inf')                        # a NaN error inside a domain is a violation, not a zero
                if (kind, name) not in self.worst or e > self.worst[(kind, name)][0]:
                    self.worst[(kind, name)] = (e, start + i, int(ops.item(b, i)))
        self.seen += n

    def report(self):
        lines = []
        for kind, name, _, arg in self.stmts:
            if kind == 'all':
                lines.append('%-10s %-26s %s' % (self.fn, name, 'holds' if name not in self.broken else
                                                 'BROKEN for %d inputs, first 0x%08x -> 0x%08x' % self.broken[name]))
            elif (kind, name) in self.worst:
                e, xb, yb = self.worst[(kind, name)]
                x = float(np.array([xb], dtype=np.uint32).view(np.float32)[0])
                lines.append('%-10s %-26s worst %s at %.9g (0x%08x -> 0x%08x), bound %g'
                             % (self.fn, name, '%.4f ulp' % e if kind == 'ulp' else '%.4e absolute' % e, x, xb, yb, arg))
        return lines

    def check(self):
        "assert every statement over what was seen"
        for kind, name, _, arg in self.stmts:
            if kind == 'all':
                assert name not in self.broken, '%s: %s: %d inputs, first 0x%08x -> 0x%08x' % ((self.fn, name) + self.broken[name])
            elif (kind, name) in self.worst:
                e, xb, yb = self.worst[(kind, name)]
                assert e <= arg, '%s: %s: %.6g %s at 0x%08x -> 0x%08x exceeds %g' % (self.fn, name, e, kind, xb, yb, arg)
