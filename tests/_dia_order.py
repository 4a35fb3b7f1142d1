"""The summation order of k_dia_mult_f64 (csrc/cgx_dia.hip), on the CPU.

An exact emulation of the order contract include/cgx.h states under "Diagonal storage", built on
tests/_spmv_order.py's ``fma`` and independent of the GPU code: every (rows per lane, diagonals in flight, load
policy, grid, device pitch) of the kernel must give these bits.

The matrix is scipy's dia_matrix, square: ``data[k, j] = A[j - offsets[k], j]``, ``data`` of shape (ndiag, ld),
ld >= n.  Row i starts from +0.0 and, for k = 0 .. ndiag-1 in stored order where 0 <= i + offsets[k] < n, does
acc = fma(data[k, i + o], v[i + o], acc).  One accumulator per row; diagonals need not be sorted, a duplicate offset
is two terms, a stored zero is a term, a row no diagonal reaches is +0.0.  Slots outside the range are never read.

``MUTATIONS``: three wrong orders (tests/test_dia_cpu.py shows that each changes bits, so the GPU test's bit-equality
tells them apart): the diagonals taken last to first, the last term added first (the accumulator not started from
+0.0), and the range test off by one (the row's last in-range column dropped).
"""
import numpy as np

from _bsmv_order import pow2_vector  # noqa: F401  (re-exported: the grid-stride test's vector)
from _spmv_order import fma

MUTATIONS = ("diagonals reversed", "last term first", "range off by one")

RS, US, POLICIES = (1, 2), (1, 2, 4, 8), (2, 8)
PLANS = tuple((R, U, nt) for R in RS for U in US for nt in POLICIES)

# The structure matrix the CPU and GPU order tests share: n odd and above 128 (more than one group of rows at both
# rows per lane, a partial last group), 17 diagonals, unsorted, offset 0 twice, the corners n-1 and -(n-1), an even
# and an odd offset beyond 64, ld = n + 3 (even, so two rows per lane take 16-byte loads).
STRUCT_N, STRUCT_LD = 131, 134
STRUCT_OFFSETS = (0, -1, 37, 2, 130, -37, 1, 0, -2, 66, -130, 67, -66, 5, -67, 12, -3)
STRUCT_NDIAGS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 17)  # prefixes: U - 1, U, U + 1 and 2 U + 1 for every U
assert len(STRUCT_OFFSETS) == 17 and STRUCT_OFFSETS.count(0) == 2
assert {1, -1, 2, -2, 37, -37, STRUCT_N - 1, 1 - STRUCT_N, 66, 67} <= set(STRUCT_OFFSETS)
assert all({U - 1, U, U + 1, 2 * U + 1} <= set(STRUCT_NDIAGS) for U in US)


def in_range(o, n):
    """The columns [lo, hi) a diagonal of offset o holds an entry of A in."""
    return max(0, o), min(n, n + o)


def structure_matrix(ndiag=17, seed=20262):
    """(offsets int32[ndiag], data (ndiag, ld), v): the first ndiag diagonals of the structure matrix; values and v
    standard normal, a few stored zeros, NaN in every slot that holds no entry of A."""
    rng = np.random.default_rng(seed)
    n, ld = STRUCT_N, STRUCT_LD
    data = rng.standard_normal((17, ld))
    data[rng.random((17, ld)) < 0.05] = 0.0  # a stored zero is a term like any other
    v = rng.standard_normal(n)
    for k, o in enumerate(STRUCT_OFFSETS):
        lo, hi = in_range(o, n)
        data[k, :lo] = np.nan
        data[k, hi:] = np.nan
    offsets = np.array(STRUCT_OFFSETS[:ndiag], np.int32)
    return offsets, np.ascontiguousarray(data[:ndiag]), v


def small_matrix(n, seed=5):
    """(offsets, data (ndiag, n + 1), v) with the offsets {0, +-1, +-2, +-(n-1)} that exist at this n, in that
    order (duplicates dropped), NaN in the unused slots."""
    offs = []
    for o in (0, 1, -1, 2, -2, n - 1, -(n - 1)):
        if -n < o < n and o not in offs:
            offs.append(o)
    rng = np.random.default_rng([seed, n])
    data = rng.standard_normal((len(offs), n + 1))
    for k, o in enumerate(offs):
        lo, hi = in_range(o, n)
        data[k, :lo] = np.nan
        data[k, hi:] = np.nan
    return np.array(offs, np.int32), data, rng.standard_normal(n)


def row(offsets, data, v, i, n, mutation=None):
    assert mutation is None or mutation in MUTATIONS
    terms = []
    for k, o in enumerate(offsets):
        j = i + int(o)
        hi = n - 1 if mutation == "range off by one" else n
        if 0 <= j < hi:
            terms.append((float(data[k][j]), float(v[j])))
    if mutation == "diagonals reversed":
        terms.reverse()
    if mutation == "last term first" and terms:
        terms = terms[-1:] + terms[:-1]
    acc = 0.0
    for a, x in terms:
        acc = fma(a, x, acc)
    return acc


def spmv_dia(offsets, data, v, n=None, mutation=None):
    """out = A v in the kernel's order, exact, row by row."""
    n = len(v) if n is None else n
    return np.array([row(offsets, data, v, i, n, mutation) for i in range(n)], dtype=np.float64).reshape(n)


def spmv_dia_pow2(offsets, data, v):
    """spmv_dia for a v of signed powers of two, vectorised over the rows: every product is exact, so an FMA is
    one correctly rounded add, which numpy does on whole arrays."""
    n = len(v)
    acc = np.zeros(n)
    for k, o in enumerate(offsets):
        lo, hi = in_range(int(o), n)  # columns; rows lo - o .. hi - o
        acc[lo - o:hi - o] = acc[lo - o:hi - o] + data[k, lo:hi] * v[lo:hi]
    return acc


def expand(offsets, data, n):
    """The scalar CSR arrays of the matrix: row i lists its entries diagonal after diagonal in stored order, in-range
    terms only, zeros included (the expansion include/cgx.h names for the preconditioners)."""
    offs = np.asarray(offsets, np.int64)
    rows = np.arange(n, dtype=np.int64)[:, None]
    cols = rows + offs[None, :]  # (n, ndiag)
    keep = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    ci = cols[keep].astype(np.int32)
    if len(offs) == 0:
        return rp, ci, np.zeros(0)
    kk = np.broadcast_to(np.arange(len(offs))[None, :], cols.shape)
    va = np.asarray(data)[kk[keep], cols[keep]].astype(np.float64)
    return rp, ci, va


def dense(offsets, data, n):
    """The explicit matrix (duplicate offsets added)."""
    A = np.zeros((n, n))
    for k, o in enumerate(offsets):
        lo, hi = in_range(int(o), n)
        j = np.arange(lo, hi)
        A[j - int(o), j] += data[k, lo:hi]
    return A


def from_dense(A, ld=None):
    """(offsets, data): every diagonal of A that holds a nonzero, offsets ascending, zero-filled (the unused slots
    too), ld = n unless given."""
    n = A.shape[0]
    assert A.shape == (n, n)
    ld = n if ld is None else ld
    offs = [o for o in range(-(n - 1), n) if np.any(np.diagonal(A, o) != 0.0)]
    data = np.zeros((len(offs), ld))
    for k, o in enumerate(offs):
        lo, hi = in_range(o, n)
        data[k, lo:hi] = np.diagonal(A, o)
    return np.array(offs, np.int32), data


def from_csr(rp, ci, va, n):
    """from_dense without the dense matrix (duplicate entries added)."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = np.asarray(ci, np.int64)
    o = cols - rows
    offs = np.unique(o[np.asarray(va) != 0.0])
    data = np.zeros((offs.size, n))
    k = np.searchsorted(offs, o)
    ok = (k < offs.size)
    ok[ok] &= offs[k[ok]] == o[ok]
    np.add.at(data, (k[ok], cols[ok]), np.asarray(va, np.float64)[ok])
    return offs.astype(np.int32), data
