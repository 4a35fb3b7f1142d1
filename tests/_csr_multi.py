"""Matrices and the numpy statement of the exchange plan for the tests of cgx_create_csr_multi (a sparse A over
equal row blocks).  numpy only -- none of it is the code under test.  Cached arrays are read-only.

The plan of a matrix over P equal row blocks (nloc = n / P rows each): block d pulls from block q != d the distinct
columns of q's row range [q nloc, (q + 1) nloc) that occur in d's rows, as ascending offsets into q's slice;
``expected_lists`` states that with np.unique."""
import functools

import numpy as np


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def from_dense(A):
    """(indptr, indices, data) of the entries of A that are not 0, row by row in column order."""
    rows, cols = np.nonzero(A)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))]).astype(np.int64)
    return _ro(indptr, cols.astype(np.int32), np.ascontiguousarray(A[rows, cols]))


@functools.lru_cache(maxsize=None)
def poisson(m):
    """The 5-point matrix of an m x m grid (4 on the diagonal, -1 to the grid neighbours), columns ascending."""
    n = m * m
    i = np.arange(n)
    r, c = np.divmod(i, m)
    A = np.zeros((n, n))
    A[i, i] = 4.0
    for ok, j in ((r > 0, i - m), (c > 0, i - 1), (c < m - 1, i + 1), (r < m - 1, i + m)):
        A[i[ok], j[ok]] = -1.0
    return from_dense(A)


@functools.lru_cache(maxsize=None)
def block_diagonal(n, P):
    """P dense diagonal blocks of n / P rows: no block names a column outside its own rows."""
    nloc = n // P
    A = np.kron(np.eye(P), np.ones((nloc, nloc))) + 4.0 * nloc * np.eye(n)
    return from_dense(A)


@functools.lru_cache(maxsize=None)
def arrowhead(n):
    """Full first row and column, and the diagonal: block 0 names every column, every block names column 0."""
    A = np.zeros((n, n))
    A[0, :] = A[:, 0] = -1.0
    A[np.arange(n), np.arange(n)] = 2.0 * n
    return from_dense(A)


def unsorted_duplicates(n=12):
    """Every row lists its columns in descending order with each one twice (values halved): the lists must come out
    ascending with every offset once.  Row i names i and (i + 5) % n, (i + 7) % n."""
    indptr = np.arange(n + 1, dtype=np.int64) * 6
    cols, vals = [], []
    for i in range(n):
        row = sorted({i, (i + 5) % n, (i + 7) % n}, reverse=True)
        assert len(row) == 3
        for j in row:
            cols += [j, j]
            vals += [4.0 if j == i else -0.5] * 2
    return _ro(indptr, np.array(cols, np.int32), np.array(vals))


def expected_lists(indptr, indices, P):
    """{(d, q): ascending offsets into block q named by block d's rows} for every pair, empty on the diagonal."""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    n = indptr.size - 1
    assert n % P == 0
    nloc = n // P
    out = {}
    for d in range(P):
        cols = np.unique(indices[indptr[d * nloc]:indptr[(d + 1) * nloc]])
        owner = cols // nloc
        for q in range(P):
            out[d, q] = (cols[owner == q] - q * nloc).astype(np.int32) if q != d else np.zeros(0, np.int32)
    return out


def expected_counts(indptr, indices, P):
    lists = expected_lists(indptr, indices, P)
    return np.array([[lists[d, q].size for q in range(P)] for d in range(P)], np.int64)
