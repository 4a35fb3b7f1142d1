"""One-sided diagonal storage of a symmetric A (cgx_set_dia_sym, csrc/cgx_dia_sym.hip), on the CPU.

The storage is scipy's dia_matrix of triu(A): offsets >= 0, ``data[k, j] = A[j - o, j]`` for j in [o, n); the stored
diagonal of offset o > 0 also stands for the diagonal -o.  The order contract (include/cgx.h "One-sided diagonal
storage") is stated against the expansion: every stored k with o > 0 becomes two consecutive diagonals, o then -o, the
mirrored one ``data'[j] = data[k, j + o]`` for j in [0, n - o); k_dia_sym_mult_f64 gives, bit for bit, what
k_dia_mult_f64 gives on that full matrix.  So the expected bits are ``_dia_order.spmv_dia(*expand(...), v)``: there is
no second emulator.

``row`` states the one-sided order directly (upper term, then lower term) only to carry the ``MUTATIONS``: three wrong
orders or slots that tests/test_dia_sym_cpu.py shows to change bits on the structure matrix, so the GPU test's
bit-equality tells them apart from the contract.
"""
import numpy as np

import _dia_order as do
from _spmv_order import fma

MUTATIONS = ("lower before upper", "lower reads the upper slot", "lower range off by one")

RS, US, POLICIES = do.RS, do.US, do.POLICIES
PLANS = do.PLANS

# The structure matrix: n odd and above 128, ld = n + 3 (even: 16-byte loads under two rows per lane), 17 stored
# diagonals, unsorted, offset 0 twice, the positive offset 37 twice, an even and an odd offset beyond 64, the corner.
STRUCT_N, STRUCT_LD = 131, 134
STRUCT_OFFSETS = (0, 37, 2, 130, 1, 0, 66, 37, 67, 5, 12, 3, 64, 129, 7, 65, 100)
STRUCT_NDIAGS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 17)  # prefixes: U - 1, U, U + 1 and 2 U + 1 for every U
assert len(STRUCT_OFFSETS) == max(STRUCT_NDIAGS) and STRUCT_OFFSETS.count(0) == 2 and STRUCT_OFFSETS.count(37) == 2
assert {1, 2, 5, 12, 37, 66, 67, STRUCT_N - 1} <= set(STRUCT_OFFSETS) and min(STRUCT_OFFSETS) == 0
assert all({U - 1, U, U + 1, 2 * U + 1} <= set(STRUCT_NDIAGS) for U in US)


def mask_unused(offsets, data, n):
    """NaN into every slot [0, o) and [n, ld) of ``data`` (in place)."""
    for k, o in enumerate(offsets):
        data[k, :int(o)] = np.nan
        data[k, n:] = np.nan
    return data


def structure_matrix(ndiag=len(STRUCT_OFFSETS), seed=20263):
    """(offsets int32[ndiag], data (ndiag, ld), v): the first ndiag stored diagonals of the structure matrix; values
    and v standard normal, a few stored zeros, NaN in every slot [0, o) and [n, ld)."""
    rng = np.random.default_rng(seed)
    n, ld, nd = STRUCT_N, STRUCT_LD, len(STRUCT_OFFSETS)
    data = rng.standard_normal((nd, ld))
    data[rng.random((nd, ld)) < 0.05] = 0.0  # a stored zero is a term like any other
    v = rng.standard_normal(n)
    mask_unused(STRUCT_OFFSETS, data, n)
    return np.array(STRUCT_OFFSETS[:ndiag], np.int32), np.ascontiguousarray(data[:ndiag]), v


def small_matrix(n, seed=6):
    """(offsets, data (ndiag, n + 1), v) with the offsets {0, 1, 2, n - 1} that exist at this n, in that order
    (duplicates dropped), NaN in the unused slots.  ld = n + 1 is odd at even n."""
    offs = []
    for o in (0, 1, 2, n - 1):
        if 0 <= o < n and o not in offs:
            offs.append(o)
    rng = np.random.default_rng([seed, n])
    data = mask_unused(offs, rng.standard_normal((len(offs), n + 1)), n)
    return np.array(offs, np.int32), data, rng.standard_normal(n)


def expand(offsets, data, n):
    """The full (offsets', data') of the contract: o then -o for every stored o > 0, a diagonal of offset 0 once.  A
    mirrored diagonal is filled in its own range [0, n - o) only; NaN everywhere else, as in the stored ones."""
    data = np.asarray(data, np.float64)
    ld = data.shape[1] if data.ndim == 2 and data.shape[0] else n
    offs, rows = [], []
    for k, o in enumerate(offsets):
        o = int(o)
        assert 0 <= o < n
        up = np.full(ld, np.nan)
        up[o:n] = data[k, o:n]
        offs.append(o)
        rows.append(up)
        if o > 0:
            low = np.full(ld, np.nan)
            low[:n - o] = data[k, o:n]
            offs.append(-o)
            rows.append(low)
    return np.array(offs, np.int32), (np.array(rows) if rows else np.zeros((0, ld)))


def upper_of(full_offsets, full_data, n):
    """The stored form of a full DIA matrix: its diagonals of offset >= 0 in their order, NaN in the slots [0, o)."""
    keep = [k for k, o in enumerate(full_offsets) if int(o) >= 0]
    offs = np.array([int(full_offsets[k]) for k in keep], np.int32)
    data = np.array([np.asarray(full_data[k], np.float64).copy() for k in keep]).reshape(len(keep), -1)
    return offs, mask_unused(offs, data, n)


def dense(offsets, data, n):
    """The explicit symmetric matrix."""
    return do.dense(*expand(offsets, data, n), n)


def row(offsets, data, v, i, n, mutation=None):
    assert mutation is None or mutation in MUTATIONS
    acc = 0.0
    for k, o in enumerate(offsets):
        o = int(o)
        if o == 0:
            acc = fma(float(data[k][i]), float(v[i]), acc)
            continue
        upper = (float(data[k][i + o]), float(v[i + o])) if i + o < n else None
        has_lower = i - o > 0 if mutation == "lower range off by one" else i - o >= 0
        lower = None
        if has_lower:
            slot = i - o if mutation == "lower reads the upper slot" else i
            a = float(data[k][slot])
            lower = (0.0 if np.isnan(a) else a, float(v[i - o]))  # the wrong slot may be an unused one
        terms = (lower, upper) if mutation == "lower before upper" else (upper, lower)
        for t in terms:
            if t is not None:
                acc = fma(t[0], t[1], acc)
    return acc


def spmv(offsets, data, v, n=None, mutation=None):
    """out = A v in the one-sided order, exact, row by row."""
    n = len(v) if n is None else n
    return np.array([row(offsets, data, v, i, n, mutation) for i in range(n)], dtype=np.float64).reshape(n)
