"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds of the project can be
compared output for output on the same arguments (the inputs are seeded).

Arrays of more than MAX_ROWS rows are cut to a fixed, seeded sample of MAX_ROWS rows; the rows kept are written next to them as
<group>_index.npy.  Every file is float32 or float64, every value in it finite, and the whole dump stays below MAX_BYTES.  The solver
reproduces the reference's NaN poisoning (a 0/0 in propagation), so the message state it returns can hold NaN: such an array is written
with its non-finite entries set to 0 and, beside it, <name>_nonfinite.npy of the same shape saying which entries they were
(0 finite, 1 NaN, 2 +inf, 3 -inf)."""
import os

import numpy as np

MAX_ROWS = 1 << 19
MAX_BYTES = 64 << 20
SAMPLE_SEED = 20251016


def sample_rows(tensors, index_name, max_rows=MAX_ROWS):
    """{name: float32 numpy array} of the torch tensors in `tensors` (all with the same number of rows), restricted to the same seeded sample
    of rows when there are more than `max_rows`; `index_name` holds the row numbers kept (float64, exact below 2**53)."""
    import torch
    n = {int(t.shape[0]) for t in tensors.values()}
    if len(n) != 1:
        raise ValueError("sample_rows: arrays of different lengths %s" % sorted(n))
    n = n.pop()
    if n <= max_rows:
        idx = np.arange(n, dtype=np.int64)
    else:
        idx = np.sort(np.random.default_rng(SAMPLE_SEED).choice(n, max_rows, replace=False))
    out = {index_name: idx.astype(np.float64)}
    for name, t in tensors.items():
        rows = t if n <= max_rows else t.index_select(0, torch.from_numpy(idx).to(t.device))
        out[name] = rows.detach().to(torch.float32).cpu().numpy()
    return out


NONFINITE_CODES = ((np.isnan, 1.0), (np.isposinf, 2.0), (np.isneginf, 3.0))


def finite_outputs(arrays):
    "the arrays with non-finite entries set to 0, plus <name>_nonfinite (0 finite, 1 NaN, 2 +inf, 3 -inf) for every array that had any"
    out = {}
    for name, a in arrays.items():
        bad = ~np.isfinite(a)
        if not bad.any():
            out[name] = a
            continue
        codes = np.zeros(a.shape, dtype=np.float32)
        for test, code in NONFINITE_CODES:
            codes[test(a)] = code
        out[name] = np.where(bad, a.dtype.type(0), a)
        out[name + '_nonfinite'] = codes
    return out


def write_outputs(directory, arrays):
    """DIR/<name>.npy for every array (float32 / float64 only), non-finite entries flagged by finite_outputs; refuses a dump above
    MAX_BYTES"""
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            raise TypeError("output %s is %s, not float32 / float64" % (name, a.dtype))
    arrays = finite_outputs(arrays)
    total = sum(a.nbytes for a in arrays.values())
    if total > MAX_BYTES:
        raise ValueError("outputs of %d bytes exceed the %d-byte limit" % (total, MAX_BYTES))
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + '.npy'), a)
    return total
