"""The summation order of k_csr_mult_f64 (cgx_csr_core.h), on the CPU.

An exact emulation of the order contract include/cgx.h states, independent of
the GPU code: every (T, load policy, grid) of the kernel must give these bits.

Row i owns the entries [s, e) = [indptr[i], indptr[i+1]) in stored order.  T
lanes share the row: sub-lane l starts from +0.0 and adds entries s+l, s+l+T,
s+l+2T, ... in that order with one fp64 FMA each; the T partial sums are then
combined as cgx_device.h's wave_sum combines 64: v[l] += v[l ^ o] for
o = T/2, ..., 1.  An empty row is +0.0.  Columns need not be sorted and a
duplicate column is two terms.
"""
from fractions import Fraction

import numpy as np

TS = (2, 4, 8, 16, 32, 64)   # the instantiated lanes per row
POLICIES = (2, 8)            # default-policy / non-temporal loads of values and col_idx

# The structure matrix the CPU and GPU order tests share: 37 rows (odd: no
# multiple of any rows-per-wave 64 / T), 200 columns, row lengths around every
# T and its multiples (one short of, equal to, one past), empty rows at the
# start, in the middle and in a run, one full-width row.
STRUCT_ROWS, STRUCT_COLS = 37, 200
STRUCT_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 131, 200, 0, 0, 1, 6,
               10, 12, 20, 0, 48, 66, 96, 130, 199, 2)
assert len(STRUCT_LENS) == STRUCT_ROWS


def structure_matrix(seed=20260):
    """(indptr, indices, data, v): columns drawn with replacement and left unsorted (duplicates occur), values and v
    standard normal."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(STRUCT_LENS)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, STRUCT_COLS, nnz).astype(np.int32)
    data = rng.standard_normal(nnz)
    v = rng.standard_normal(STRUCT_COLS)
    return indptr, indices, data, v


def fma(a, b, c):
    """a * b + c with one rounding: the Fractions are exact, float() of one rounds correctly."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def butterfly(v):
    """v[l] += v[l ^ o] for o = len(v) / 2, ..., 1; every lane ends with the same bits."""
    v = [float(x) for x in v]
    o = len(v) // 2
    while o:
        v = [v[l] + v[l ^ o] for l in range(len(v))]
        o >>= 1
    assert all(x == v[0] or x != x for x in v)
    return v[0]


def spmv_row(indices, data, v, T):
    """One row's sum from its entries in stored order."""
    lanes = []
    for l in range(T):
        acc = 0.0
        for e in range(l, len(data), T):
            acc = fma(float(data[e]), float(v[int(indices[e])]), acc)
        lanes.append(acc)
    return butterfly(lanes)


def spmv_csr(indptr, indices, data, v, T):
    assert T in TS
    n = len(indptr) - 1
    out = np.empty(n)
    for i in range(n):
        s, e = int(indptr[i]), int(indptr[i + 1])
        out[i] = spmv_row(indices[s:e], data[s:e], v, T)
    return out


def _butterfly64(lanes):
    """wave_sum on every row of an (m, 64) array: lanes[:, l] += lanes[:, l ^ o] for o = 32, ..., 1."""
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o >>= 1
    return lanes[:, 0]


def fused_dot(out, p, T, blocks):
    """The kernel's fused dot p . out on a grid of `blocks` blocks of 4 waves, for terms p[i] * out[i] that are
    exact in fp64 (p signed powers of two), so that every step is one correctly rounded add.  Wave w of the grid
    takes the row groups w, w + 4 blocks, ...; the lane that stores row i of a group adds its term to its own sum
    (from +0.0, in that order); then wave_sum, the block's four waves in order, and grid_sum_last_block's sum of the
    block totals: one block stores 0.0 + its total; otherwise thread t of the last block adds the totals t, t + 256,
    ... in that order, then wave_sum and the four waves in order again."""
    RW, W = 64 // T, 4 * blocks
    term = np.asarray(p, np.float64) * out
    sweeps = -(-(-(-term.size // RW)) // W)
    rows = np.zeros(sweeps * W * RW)
    rows[:term.size] = term
    acc = np.zeros((W, RW))
    for part in rows.reshape(sweeps, W, RW):
        acc = acc + part
    lanes = np.zeros((W, 64))
    lanes[:, ::T] = acc  # the storing lane of row r of the group is lane r T
    red = _butterfly64(lanes).reshape(blocks, 4)
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    if blocks == 1:
        return 0.0 + tot[0]
    assert blocks <= 8192
    s = np.zeros(256)
    for i0 in range(0, blocks, 256):
        s[:tot[i0:i0 + 256].size] += tot[i0:i0 + 256]
    red = _butterfly64(s.reshape(4, 64))
    return ((red[0] + red[1]) + red[2]) + red[3]


def exact_rows(indptr, indices, data, v):
    """Per row: (the correctly rounded exact sum, sum of |terms| as a float, the entry count)."""
    res = []
    for i in range(len(indptr) - 1):
        s, e = int(indptr[i]), int(indptr[i + 1])
        terms = [Fraction(float(data[k])) * Fraction(float(v[int(indices[k])])) for k in range(s, e)]
        res.append((float(sum(terms, Fraction(0))), float(sum((abs(t) for t in terms), Fraction(0))), e - s))
    return res


def tridiag(n):
    """The tridiagonal matrix of the grid-stride test: row i holds columns (i-1, i, i+1) inside [0, n), in that
    order.  Every value is a signed power of two, so each product values[e] * v[col] is exact in fp64 and an FMA
    onto an accumulator is one correctly rounded add, which numpy can do on whole arrays (spmv_tridiag); the sums
    still round, so their order shows in the bits.  (Not symmetric: this is a matVec test.)"""
    i = np.arange(n, dtype=np.int64)
    cols = np.stack([i - 1, i, i + 1], axis=1)
    vals = np.stack([-(0.5 ** (i % 3)), 2.0 ** (1 + i % 2), -(0.5 ** (i % 4))], axis=1)
    keep = (cols >= 0) & (cols < n)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return indptr, cols[keep].astype(np.int32), vals[keep]


def spmv_tridiag(n, v, T, csr=None):
    """spmv_csr on tridiag(n), vectorised over the rows.  A row has at most 3 entries: with T >= 4 every sub-lane
    holds at most one (exact) product, with T = 2 sub-lane 0 holds entry 0 and then entry 2.  csr: a matrix of
    tridiag(n)'s structure with other values, for a v that keeps the products exact."""
    indptr, indices, data = csr or tridiag(n)
    lens = np.diff(indptr)
    prod = np.zeros((n, 3))  # the exact product of entry k of row i, +0.0 where the row is shorter
    for k in range(3):
        has = lens > k
        e = indptr[:-1][has] + k
        prod[has, k] = data[e] * v[indices[e]]
    lane = np.zeros((n, T))
    if T == 2:
        lane[:, 0] = (0.0 + prod[:, 0]) + prod[:, 2]
        lane[:, 1] = 0.0 + prod[:, 1]
    else:
        lane[:, :3] = 0.0 + prod
    o = T // 2
    while o:
        lane = lane + lane[:, np.arange(T) ^ o]
        o >>= 1
    return lane[:, 0]
