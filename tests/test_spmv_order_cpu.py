"""The CPU statement of k_csr_mult_f64's summation order (tests/_spmv_order.py), checked against exact
arithmetic, so the GPU test (test_gpu_csr.py) compares the kernel with something that is itself verified."""
import math

import numpy as np
import pytest

import _spmv_order as so


@pytest.fixture(scope="module")
def struct():
    return so.structure_matrix()


@pytest.fixture(scope="module")
def by_T(struct):
    return {T: so.spmv_csr(*struct, T) for T in so.TS}


def test_structure_matrix_shape(struct):
    indptr, indices, data, v = struct
    assert len(indptr) == so.STRUCT_ROWS + 1 == 38 and v.size == so.STRUCT_COLS == 200
    assert tuple(np.diff(indptr)) == so.STRUCT_LENS
    assert tuple(so.STRUCT_LENS[:27]) == (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128,
                                          129, 131, 200, 0, 0, 1, 6)
    assert indices.min() >= 0 and indices.max() < so.STRUCT_COLS
    # unsorted rows and duplicate columns both occur
    rows = [indices[indptr[i]:indptr[i + 1]] for i in range(so.STRUCT_ROWS)]
    assert any(np.any(np.diff(r) < 0) for r in rows)
    assert any(np.unique(r).size < r.size for r in rows)


@pytest.mark.parametrize("T", so.TS)
def test_emulation_within_rounding_of_the_exact_sum(struct, by_T, T):
    """Each row within len * 2^-53 * sum |terms| of the correctly rounded exact sum: len - 1 + log2(T) roundings at
    the most touch a term (its FMA chain, then the butterfly), each at most 2^-53 relative to a partial sum that
    sum |terms| bounds; one more for the rounding of the exact sum itself."""
    for i, (exact, mag, cnt) in enumerate(so.exact_rows(*struct)):
        bound = max(cnt, 1) * 2.0 ** -53 * mag
        assert abs(by_T[T][i] - exact) <= bound, (T, i, by_T[T][i], exact, bound)


@pytest.mark.parametrize("T", so.TS)
def test_empty_row_is_plus_zero(by_T, T):
    for i, ln in enumerate(so.STRUCT_LENS):
        if ln == 0:
            assert by_T[T][i] == 0.0 and not np.signbit(by_T[T][i])
    indptr = np.array([0, 0, 0], np.int64)
    out = so.spmv_csr(indptr, np.zeros(0, np.int32), np.zeros(0), np.ones(3), T)
    assert np.array_equal(out, [0.0, 0.0]) and not np.signbit(out).any()


def test_plans_can_be_told_apart(by_T):
    """T = 2 and T = 64 differ in at least one row's bits, so a GPU run under the wrong T would be seen."""
    assert np.any(by_T[2] != by_T[64])
    # ... and rows no longer than 2 entries are the same under every T (one product per sub-lane)
    short = [i for i, ln in enumerate(so.STRUCT_LENS) if ln <= 2]
    for T in so.TS:
        assert np.array_equal(by_T[T][short], by_T[2][short])


def test_duplicates_and_stored_order_are_honoured():
    indptr = np.array([0, 3], np.int64)
    indices = np.array([1, 1, 0], np.int32)
    data = np.array([1e16, 1.0, -1e16])
    v = np.array([1.0, 1.0])
    # T = 2: sub-lane 0 takes entries 0 and 2 (1e16 - 1e16 = 0), sub-lane 1 entry 1: 0 + 1
    assert so.spmv_csr(indptr, indices, data, v, 2)[0] == 1.0
    # stored the other way round, sub-lane 0 adds 1e16 + 1 first (lost), then sub-lane 1's -1e16
    assert so.spmv_csr(indptr, np.array([1, 0, 1], np.int32), np.array([1e16, -1e16, 1.0]), v, 2)[0] == 0.0


@pytest.mark.parametrize("T", (2, 8, 64))
def test_vectorised_tridiagonal_emulation_equals_the_general_one(T):
    n = 203
    v = np.random.default_rng(5).standard_normal(n)
    want = so.spmv_csr(*so.tridiag(n), v, T)
    got = so.spmv_tridiag(n, v, T)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    assert tuple(np.diff(so.tridiag(n)[0])[[0, 1, -1]]) == (2, 3, 2)
    assert so.spmv_tridiag(1, v[:1], T)[0] == so.spmv_csr(*so.tridiag(1), v[:1], T)[0] == 2.0 * v[0]


@pytest.mark.parametrize("T,blocks,n", [(8, 1, 29), (8, 3, 1000), (2, 300, 70001), (64, 2048, 9000)])
def test_fused_dot_counts_every_row_once_and_shows_the_order(T, blocks, n):
    rng = np.random.default_rng(n)
    p = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-1, 2, n)
    whole = rng.integers(-1000, 1000, n).astype(np.float64)  # every partial sum is exact: the order cannot show
    assert so.fused_dot(whole, p, T, blocks) == float(np.sum(p * whole))
    out = rng.standard_normal(n)
    got = so.fused_dot(out, p, T, blocks)
    assert abs(got - math.fsum(p * out)) <= 2.0 ** -52 * n * float(np.abs(p * out).max())
    if n > 1000:  # another grid is another order
        assert got != so.fused_dot(out, p, T, blocks + 1) or got != so.fused_dot(out, p, T, blocks + 2)


def test_tridiagonal_emulation_with_other_values():
    n, T = 203, 8
    rng = np.random.default_rng(6)
    indptr, indices, _ = so.tridiag(n)
    csr = (indptr, indices, rng.standard_normal(indices.size))
    v = 2.0 ** rng.integers(-1, 2, n)
    assert np.array_equal(so.spmv_tridiag(n, v, T, csr), so.spmv_csr(*csr, v, T))
