"""tests/_bsmv_order.py checked on the CPU: the emulation of k_bsr_mult_f64's summation order agrees with itself across
T to rounding, equals a hand-computed chain where there is only one, and tells the three wrong orders of
``MUTATIONS`` apart by their bits -- so the GPU test's bit-equality (tests/test_gpu_bsr.py) means the order.  The two
probe modules' bars at the sizes the GPU probe of the block-valued iteration uses are asserted here too."""
import functools
import time

import numpy as np
import pytest

import _bsmv_order as bo
import _nrhs_probe as npr
import _pcg_probe as pp
from _spmv_order import fma


@functools.lru_cache(maxsize=None)
def struct(bs):
    return bo.structure_matrix(bs)


@functools.lru_cache(maxsize=None)
def expected(bs, T):
    return bo.spmv_bsr(*struct(bs), T)


def test_structure_matrix_shape():
    for bs in bo.BLOCK_SIZES:
        indptr, indices, data, v = struct(bs)
        assert indptr.size == bo.STRUCT_NB + 1 and data.shape == (indices.size, bs, bs) and v.size == bo.STRUCT_NCOLB * bs
        assert tuple(np.diff(indptr)) == bo.STRUCT_LENS and np.any(data == 0.0)
        assert 0 <= indices.min() and indices.max() < bo.STRUCT_NCOLB


def test_all_block_sizes_and_T_emulate_quickly():
    t0 = time.perf_counter()
    for bs in bo.BLOCK_SIZES:
        for T in bo.TS:
            expected(bs, T)
    assert time.perf_counter() - t0 < 60.0


@pytest.mark.parametrize("bs", bo.BLOCK_SIZES)
def test_T_independence_to_rounding(bs):
    """Every T sums the same terms: the results agree with the dense product to rounding, and the bits do differ
    between some pair of T (the order is visible at all)."""
    indptr, indices, data, v = struct(bs)
    A = bo.dense(indptr, indices, data, bo.STRUCT_NCOLB)
    ref, scale = A @ v, np.abs(A) @ np.abs(v)
    outs = [expected(bs, T) for T in bo.TS]
    live = scale > 0
    for out in outs:
        assert np.all(np.abs(out - ref)[live] <= 64 * np.finfo(float).eps * scale[live])
        assert np.all(out[~live] == 0.0) and not np.any(np.signbit(out[~live]))  # an empty block row: +0.0
    assert any(not np.array_equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize("bs", bo.BLOCK_SIZES)
def test_one_diagonal_block_per_row_is_the_hand_chain(bs):
    """One block per block row, on the diagonal: sub-lane 0 holds the whole chain, every other sub-lane +0.0, and
    adding +0.0 changes nothing (no sum here is -0.0), so each row is fma(B[i][bs-1], v[bs-1], ... fma(B[i][0],
    v[0], +0.0))."""
    nb = 5
    rng = np.random.default_rng([bs, 3])
    indptr = np.arange(nb + 1, dtype=np.int64)
    indices = np.arange(nb, dtype=np.int32)
    data, v = rng.standard_normal((nb, bs, bs)), rng.standard_normal(nb * bs)
    want = np.empty(nb * bs)
    for I in range(nb):
        for i in range(bs):
            acc = 0.0
            for j in range(bs):
                acc = fma(float(data[I, i, j]), float(v[I * bs + j]), acc)
            want[I * bs + i] = acc
    for T in bo.TS:
        assert np.array_equal(bo.spmv_bsr(indptr, indices, data, v, T), want)


@pytest.mark.parametrize("mutation", bo.MUTATIONS)
@pytest.mark.parametrize("bs", [2, 3, 8])
def test_mutations_change_bits(bs, mutation):
    # at T = 2 the butterfly is one commutative add: its reversal is the same order
    for T in ((4, 8, 64) if mutation == "butterfly reversed" else (2, 8, 64)):
        good, bad = expected(bs, T), bo.spmv_bsr(*struct(bs), T, mutation)
        assert not np.array_equal(good, bad), (bs, T, mutation)


def test_expansion_is_the_same_matrix():
    from _spmv_order import spmv_csr
    indptr, indices, data, v = struct(3)
    rp, ci, va = bo.expand(indptr, indices, data)
    assert rp[-1] == indices.size * 9 and rp.size == bo.STRUCT_NB * 3 + 1
    A = np.zeros((bo.STRUCT_NB * 3, bo.STRUCT_NCOLB * 3))
    np.add.at(A, (np.repeat(np.arange(rp.size - 1), np.diff(rp)), ci), va)
    assert np.array_equal(A, bo.dense(indptr, indices, data, bo.STRUCT_NCOLB))
    # the same terms in another order (CSR deals single entries to the sub-lanes): equal to rounding, not in bits
    out = spmv_csr(rp, ci, va, v, 8)
    assert np.allclose(out, expected(3, 8), rtol=0, atol=1e-12)


def test_from_dense_round_trip():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((12, 12)) * (rng.random((12, 12)) < 0.2)
    for bs in (2, 3, 4, 6):
        indptr, indices, data = bo.from_dense(A, bs)
        assert np.array_equal(bo.dense(indptr, indices, data), A)
        assert all(np.any(blk != 0.0) for blk in data)


@pytest.mark.parametrize("bs,T", [(2, 2), (3, 2), (8, 2), (2, 64), (3, 64), (8, 64), (3, 4), (3, 8)])
def test_vectorised_block_tridiag_is_the_emulation(bs, T):
    nb = 9
    v = bo.pow2_vector(nb * bs)
    want = bo.spmv_bsr(*bo.block_tridiag(nb, bs), v, T)
    assert np.array_equal(bo.spmv_block_tridiag(nb, bs, v, T), want)


@pytest.mark.parametrize("bs", [2, 3, 8])
def test_block_tridiag_sums_do_round(bs):
    """The products are exact but the sums round, so the order shows: T = 2 (blocks 0 and 2 in one chain) and T = 64
    (one block per sub-lane) differ in bits on many rows."""
    nb = 2001
    v = bo.pow2_vector(nb * bs)
    a, b = bo.spmv_block_tridiag(nb, bs, v, 2), bo.spmv_block_tridiag(nb, bs, v, 64)
    assert np.count_nonzero(a != b) >= nb * bs // 10, np.count_nonzero(a != b)


# ---- the probe bars the GPU test rests on --------------------------------------------------------------------------
def probe_sizes(bs):
    """The smallest multiples of bs that are >= 257 and >= 2049."""
    return tuple(-(-m // bs) * bs for m in (257, 2049))


def test_probe_sizes():
    assert probe_sizes(2) == (258, 2050) and probe_sizes(7) == (259, 2051) and probe_sizes(8) == (264, 2056)


@pytest.mark.parametrize("bs", bo.BLOCK_SIZES)
def test_probe_bars_stay_under_the_cap(bs):
    for n in probe_sizes(bs):
        for zero in (False, True):
            col = npr.Col("csr", n, 0, zero)
            for k in npr.KS:
                assert npr.FLOOR * 100 <= npr.bar(col, k) <= npr.CAP
            for k in npr.rr_loops(n):
                assert npr.FLOOR * 100 <= npr.rr_bar(col, k) <= npr.CAP
            for kind, b in (("jacobi", 0), ("diag", 0), ("block", bs)):
                case = pp.Case(kind, b, n, zero)
                for k in pp.KS:
                    assert pp.FLOOR * 100 <= pp.bar(case, k) <= pp.CAP
