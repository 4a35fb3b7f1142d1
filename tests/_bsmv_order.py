"""The summation order of k_bsr_mult_f64 (csrc/cgx_bsmv.hip), on the CPU.

An exact emulation of the order contract include/cgx.h states under "Block storage", built on tests/_spmv_order.py's
``fma`` and ``butterfly`` and independent of the GPU code: every (T, load policy, grid, device layout) of the kernel
must give these bits.

Block row I owns the blocks [s, e) = [indptr[I], indptr[I+1]) in stored order, each a dense bs x bs block, row-major.
T lanes share the block row.  For scalar row I bs + i, sub-lane l starts from +0.0 and, for each of its blocks s+l,
s+l+T, s+l+2T, ... in that order and j = 0 .. bs-1 ascending inside a block in block column c, does
acc_i = fma(B[i][j], v[c bs + j], acc_i); the T partial sums are then combined as v[l] += v[l ^ o] for
o = T/2, ..., 1.  An empty block row is bs values of +0.0.  Block columns need not be sorted, a duplicate block column
is two terms and a stored zero is a term.

``MUTATIONS``: three wrong orders (tests/test_bsmv_order_cpu.py shows that each changes bits, so the GPU test's
bit-equality tells them apart): j descending inside a block, sub-lane l taking the blocks l, l + T + 1, ..., and the
butterfly run as o = 1, ..., T/2.
"""
import numpy as np

from _spmv_order import POLICIES, TS, butterfly, fma  # noqa: F401  (re-exported: the order tests' parameters)

BLOCK_SIZES = tuple(range(2, 9))
MUTATIONS = ("j descending", "lane stride T+1", "butterfly reversed")

# The structure matrix the CPU and GPU order tests share: 23 block rows (odd: no multiple of any block rows per wave
# 64 / T), 40 block columns; the block-row lengths are 0, 1, T - 1, T, T + 1 and 2 T + 1 for every T, with a run of
# three empty block rows.  510 blocks: at bs = 8, 32,640 FMAs per T.
STRUCT_NB, STRUCT_NCOLB = 23, 40
STRUCT_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 0, 0, 0, 6)
assert len(STRUCT_LENS) == STRUCT_NB and STRUCT_NB % 2 == 1
assert all({0, 1, T - 1, T, T + 1, 2 * T + 1} <= set(STRUCT_LENS) for T in TS)


def structure_matrix(bs, seed=20261):
    """(indptr, indices, data of shape (nnzb, bs, bs), v): block columns drawn with replacement and left unsorted
    (duplicates occur), values and v standard normal, a few stored zeros among the values."""
    rng = np.random.default_rng([seed, bs])
    indptr = np.concatenate([[0], np.cumsum(STRUCT_LENS)]).astype(np.int64)
    nnzb = int(indptr[-1])
    indices = rng.integers(0, STRUCT_NCOLB, nnzb).astype(np.int32)
    data = rng.standard_normal((nnzb, bs, bs))
    data[rng.random((nnzb, bs, bs)) < 0.03] = 0.0  # a stored zero is a term like any other
    v = rng.standard_normal(STRUCT_NCOLB * bs)
    for I in range(STRUCT_NB):  # the draw does hold duplicates and unsorted columns
        c = indices[indptr[I]:indptr[I + 1]]
        if c.size >= 63:
            assert np.unique(c).size < c.size and np.any(np.diff(c) < 0)
    return indptr, indices, data, v


def _butterfly_reversed(v):
    v = [float(x) for x in v]
    o = 1
    while o < len(v):
        v = [v[l] + v[l ^ o] for l in range(len(v))]
        o <<= 1
    return v[0]


def block_row(cols, blocks, v, bs, T, mutation=None):
    """The bs sums of one block row from its blocks in stored order."""
    assert mutation is None or mutation in MUTATIONS
    stride = T + 1 if mutation == "lane stride T+1" else T
    js = range(bs - 1, -1, -1) if mutation == "j descending" else range(bs)
    lanes = []
    for l in range(T):
        acc = [0.0] * bs
        for q in range(l, len(cols), stride):
            base = int(cols[q]) * bs
            for i in range(bs):
                a = acc[i]
                for j in js:
                    a = fma(float(blocks[q][i][j]), float(v[base + j]), a)
                acc[i] = a
        lanes.append(acc)
    combine = _butterfly_reversed if mutation == "butterfly reversed" else butterfly
    return [combine([lanes[l][i] for l in range(T)]) for i in range(bs)]


def spmv_bsr(indptr, indices, data, v, T, mutation=None):
    assert T in TS
    nb, bs = len(indptr) - 1, data.shape[1]
    out = np.empty(nb * bs)
    for I in range(nb):
        s, e = int(indptr[I]), int(indptr[I + 1])
        out[I * bs:(I + 1) * bs] = block_row(indices[s:e], data[s:e], v, bs, T, mutation)
    return out


def expand(indptr, indices, data):
    """The scalar CSR arrays of a BSR matrix: row I bs + i lists its entries block after block in stored order, j
    ascending inside a block, zeros included (the expansion include/cgx.h names for the preconditioners)."""
    nb, bs = len(indptr) - 1, data.shape[1]
    lens = np.repeat(np.diff(indptr), bs) * bs
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.empty(int(rp[-1]), np.int32)
    va = np.empty(int(rp[-1]))
    for I in range(nb):
        s, e = int(indptr[I]), int(indptr[I + 1])
        cols = (indices[s:e, None].astype(np.int64) * bs + np.arange(bs)[None, :]).reshape(-1)
        for i in range(bs):
            r = I * bs + i
            ci[rp[r]:rp[r + 1]] = cols
            va[rp[r]:rp[r + 1]] = data[s:e, i, :].reshape(-1)
    return rp, ci, va


def dense(indptr, indices, data, ncolb=None):
    """The explicit matrix (duplicate blocks added)."""
    nb, bs = len(indptr) - 1, data.shape[1]
    A = np.zeros((nb * bs, (ncolb or nb) * bs))
    for I in range(nb):
        for q in range(int(indptr[I]), int(indptr[I + 1])):
            c = int(indices[q])
            A[I * bs:(I + 1) * bs, c * bs:(c + 1) * bs] += data[q]
    return A


def from_dense(A, bs):
    """(indptr, indices, data): every bs x bs block of A that holds a nonzero, block columns ascending, the blocks'
    other entries zero-filled."""
    n = A.shape[0]
    assert A.shape == (n, n) and n % bs == 0
    nb = n // bs
    B = A.reshape(nb, bs, nb, bs).transpose(0, 2, 1, 3)
    keep = np.any(B != 0.0, axis=(2, 3))
    rows, cols = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nb))]).astype(np.int64)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(B[rows, cols])


# ---- the grid-stride test's matrix: block tridiagonal, multiplied by signed powers of two ---------------------------
def block_tridiag(nb, bs, seed=13):
    """Block row I holds the block columns (I-1, I, I+1) inside [0, nb), in that order; the values are standard
    normal.  (Not symmetric: this is a matVec test.)"""
    I = np.arange(nb, dtype=np.int64)
    cols = np.stack([I - 1, I, I + 1], axis=1)
    keep = (cols >= 0) & (cols < nb)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    indices = cols[keep].astype(np.int32)
    data = np.random.default_rng([seed, nb, bs]).standard_normal((indices.size, bs, bs))
    return indptr, indices, data


def pow2_vector(n, seed=11):
    """Signed powers of two, 2^-8 .. 2^8: every product B[i][j] * v[k] is exact in fp64, so an FMA onto an
    accumulator is one correctly rounded add, which numpy does on whole arrays (spmv_block_tridiag); the sums still
    round, so their order shows in the bits."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(-8, 9, n)


def spmv_block_tridiag(nb, bs, v, T):
    """spmv_bsr on block_tridiag(nb, bs) for a v of signed powers of two, vectorised over the block rows.  A block
    row has at most 3 blocks: with T >= 4 sub-lane k holds block k alone, with T = 2 sub-lane 0 holds block 0 and
    then block 2, sub-lane 1 block 1.  Sub-lanes past the third hold +0.0: adding them leaves lanes 0..3 as
    x + 0.0, after which the butterfly is the one of four lanes."""
    indptr, indices, data = block_tridiag(nb, bs)
    lens = np.diff(indptr)
    V = v.reshape(nb, bs)

    def chain(acc, k):
        """acc (nb, bs) after block k of every block row that has one: j ascending, one rounded add per product."""
        has = lens > k
        q = indptr[:-1][has] + k
        a = acc[has]
        for j in range(bs):
            a = a + data[q, :, j] * V[indices[q], j][:, None]
        acc = acc.copy()
        acc[has] = a
        return acc

    zero = np.zeros((nb, bs))
    if T == 2:
        lanes = [chain(chain(zero, 0), 2), chain(zero, 1)]
    else:
        lanes = [chain(zero, 0), chain(zero, 1), chain(zero, 2), zero]
        if T > 4:
            lanes = [x + 0.0 for x in lanes]
    while len(lanes) > 1:  # v[l] += v[l ^ o], o = len / 2, ..., 1
        o = len(lanes) // 2
        lanes = [lanes[l] + lanes[l ^ o] for l in range(o)]
    return lanes[0].reshape(-1)
