"""cgx_create_csr_multi without a GPU: the exchange plan (cgx_csr_halo_counts / cgx_csr_halo_list, the builder
cgx_set_csr runs) against its numpy statement (tests/_csr_multi.py: np.unique of each block's out-of-block columns,
split by owner), the argument checks that run before any device is touched, and the Python mirror's own checks."""
import ctypes

import numpy as np
import pytest

import _csr_multi as cm
import conjugate_gradient_amd as cg
from test_gpu_csr_nrhs import masked

# None on a tree without the feature: every test then fails at its first use
halo_counts = getattr(cg, "csr_halo_counts", None)
halo_list = getattr(cg, "csr_halo_list", None)
HALO_ACTIVE = getattr(cg, "CGX_CSR_HALO_ACTIVE", None)

ERR_ARG, ERR_SHAPE = -1, -4
REFUSED = ("CGX_F32_REF", "CGX_A_F32", "CGX_SYMMETRIC", "CGX_HOST_STREAM", "CGX_PHASES", "CGX_COMM_P2P",
           "CGX_NO_OVERLAP", "CGX_DETERMINISTIC")


@pytest.fixture(scope="module")
def L(built):
    return cg.lib()


def _p(a):
    return a.ctypes.data


def _err(L):
    return L.cgx_last_error().decode()


def held_to_numpy(indptr, indices, P):
    """Every (dst, src) list and the counts against the numpy statement; returns the lists."""
    want = cm.expected_lists(indptr, indices, P)
    counts = halo_counts(indptr, indices, P)
    assert counts.dtype == np.int64 and np.array_equal(counts, cm.expected_counts(indptr, indices, P))
    for (d, q), w in want.items():
        got = halo_list(indptr, indices, P, d, q)
        assert got.dtype == np.int32 and np.array_equal(got, w), (P, d, q, got, w)
        assert np.all(np.diff(got) > 0)  # ascending, each offset once
    assert all(want[d, d].size == 0 for d in range(P))
    return want


@pytest.mark.parametrize("n,seed,P", [(1000, 2, 1), (1000, 2, 2), (1000, 2, 4), (1000, 2, 8), (2100, 8, 3),
                                      (2100, 8, 4)])
def test_lists_of_the_masked_matrices(built, n, seed, P):
    indptr, indices, _ = masked(n, seed)[1]
    want = held_to_numpy(indptr, indices, P)
    if P > 1:  # the rows and columns at multiples of 50 reach every block
        assert all(want[d, q].size > 0 for d in range(P) for q in range(P) if d != q)


@pytest.mark.parametrize("P", [2, 3, 4, 6])
def test_lists_of_the_poisson_matrix(built, P):
    indptr, indices, _ = cm.poisson(12)
    want = held_to_numpy(indptr, indices, P)
    nloc = 144 // P
    for d in range(P):
        for q in range(P):  # one grid row of 12 from each neighbouring block, nothing from any other
            near = abs(d - q) == 1
            assert want[d, q].size == (12 if near else 0)
            if near:
                first = nloc - 12 if q < d else 0
                assert np.array_equal(want[d, q], np.arange(first, first + 12))
    if P == 2:
        assert np.array_equal(halo_list(indptr, indices, 2, 0, 1), np.arange(0, 12))
        assert np.array_equal(halo_list(indptr, indices, 2, 1, 0), np.arange(60, 72))


def test_block_diagonal_has_empty_lists(built):
    indptr, indices, _ = cm.block_diagonal(24, 4)
    want = held_to_numpy(indptr, indices, 4)
    assert all(w.size == 0 for w in want.values())
    assert not halo_counts(indptr, indices, 4).any()
    assert halo_counts(indptr, indices, 2).tolist() == [[0, 0], [0, 0]]  # two diagonal blocks per row block


def test_arrowhead_lists_are_whole_slices(built):
    indptr, indices, _ = cm.arrowhead(20)
    want = held_to_numpy(indptr, indices, 4)
    for q in range(1, 4):
        assert np.array_equal(want[0, q], np.arange(5))  # the full first row: all of every other block
        assert np.array_equal(want[q, 0], [0])  # the full first column: entry 0 of block 0
    # one row per block: the list into and out of block 0 is the whole one-row slice
    want = held_to_numpy(indptr, indices, 20)
    assert all(np.array_equal(want[0, q], [0]) and np.array_equal(want[q, 0], [0]) for q in range(1, 20))
    assert all(want[d, q].size == 0 for d in range(1, 20) for q in range(1, 20))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 12])
def test_unsorted_and_duplicate_columns(built, P):
    indptr, indices, _ = cm.unsorted_duplicates(12)
    assert not np.all(np.diff(indices[:6]) >= 0)  # the rows really are out of order
    held_to_numpy(indptr, indices, P)


def test_one_block_has_one_zero_count(built):
    indptr, indices, _ = cm.poisson(12)
    assert halo_counts(indptr, indices, 1).tolist() == [[0]]
    assert halo_list(indptr, indices, 1, 0, 0).size == 0


# ---- the host-only calls' own refusals ----------------------------------------------------------------------
def test_halo_calls_run_the_structure_check_first(L):
    rp = np.array([0, 0, 3, 4, 8], np.int64)
    out = np.full(4, -7, np.int64)
    for ci, named in (([3, 0, 3, 1, 0, 1, 2, 4], "col_idx[7] = 4"), ([3, 0, 3, 1, 0, -1, 2, 3], "col_idx[5] = -1")):
        ci = np.array(ci, np.int32)
        assert L.cgx_csr_halo_counts(4, 2, _p(rp), _p(ci), _p(out)) == ERR_SHAPE
        assert "cgx_csr_check" in _err(L) and named in _err(L), _err(L)
        lst = np.full(4, -7, np.int32)
        assert L.cgx_csr_halo_list(4, 2, _p(rp), _p(ci), 0, 1, _p(lst)) == ERR_SHAPE
        assert "cgx_csr_check" in _err(L) and named in _err(L), _err(L)
        assert np.all(out == -7) and np.all(lst == -7)  # nothing written
        with pytest.raises(cg.CgxError) as e:
            halo_counts(rp, ci, 2)
        assert e.value.code == ERR_SHAPE and named in str(e.value)
    bad = np.array([0, 3, 2, 4, 8], np.int64)
    ci = np.array([3, 0, 3, 1, 0, 1, 2, 3], np.int32)
    assert L.cgx_csr_halo_counts(4, 2, _p(bad), _p(ci), _p(out)) == ERR_SHAPE and "decreases at row 1" in _err(L)


def test_halo_calls_refuse_bad_partitions_and_pointers(L):
    rp = np.array([0, 0, 3, 4, 8], np.int64)
    ci = np.array([3, 0, 3, 1, 0, 1, 2, 3], np.int32)
    out = np.zeros(33 * 33, np.int64)
    assert L.cgx_csr_halo_counts(4, 3, _p(rp), _p(ci), _p(out)) == ERR_SHAPE and "not divisible" in _err(L)
    for P in (0, -1, 33):
        assert L.cgx_csr_halo_counts(4, P, _p(rp), _p(ci), _p(out)) == ERR_ARG and "nshards" in _err(L)
    assert L.cgx_csr_halo_counts(0, 1, _p(rp), _p(ci), _p(out)) == ERR_ARG
    assert L.cgx_csr_halo_counts(4, 2, None, _p(ci), _p(out)) == ERR_ARG
    assert L.cgx_csr_halo_counts(4, 2, _p(rp), None, _p(out)) == ERR_ARG
    assert L.cgx_csr_halo_counts(4, 2, _p(rp), _p(ci), None) == ERR_ARG
    lst = np.zeros(4, np.int32)
    for d, s in ((-1, 0), (2, 0), (0, 2), (0, -1)):
        assert L.cgx_csr_halo_list(4, 2, _p(rp), _p(ci), d, s, _p(lst)) == ERR_ARG, (d, s)
    assert L.cgx_get_csr_halo(None, _p(out)) == ERR_ARG
    assert L.cgx_gather_indexed(None, None, 0, None, None) == 0  # nothing to move: nothing is touched
    assert L.cgx_gather_indexed(None, None, 3, None, None) == ERR_ARG
    assert L.cgx_gather_indexed(None, None, -1, None, None) == ERR_SHAPE


# ---- cgx_create_csr_multi: refused before any device is touched ---------------------------------------------
def _create(L, n, nnz_block, nshards, flags, devices=(0,) * 33):
    h = ctypes.c_void_p(0xdead)  # must come back NULL on every refusal
    arr = (ctypes.c_int * len(devices))(*devices)
    return L.cgx_create_csr_multi(ctypes.byref(h), n, nnz_block, nshards, arr, flags), h.value


def test_create_refuses_a_partition_that_does_not_divide(L):
    for n, P in ((10, 3), (1000, 7), (31, 32)):
        rc, h = _create(L, n, 5, P, cg.CGX_F64)
        assert rc == ERR_SHAPE and h is None, (n, P, rc, h)
        assert "cgx_create_csr_multi" in _err(L) and "not divisible" in _err(L)


def test_create_refuses_block_counts_and_sizes(L):
    for P in (0, 33, -2):
        rc, h = _create(L, 1056, 5, P, cg.CGX_F64)
        assert rc == ERR_ARG and h is None and "nshards" in _err(L), (P, rc, h, _err(L))
    for n, nnz in ((0, 5), (-4, 5), (2 ** 31, 5), (8, -1)):
        rc, h = _create(L, n, nnz, 2, cg.CGX_F64)
        assert rc == ERR_ARG and h is None and "cgx_create_csr_multi" in _err(L), (n, nnz, rc, h)


@pytest.mark.parametrize("name", REFUSED)
@pytest.mark.parametrize("timing", [0, cg.CGX_TIMING])
def test_create_refuses_every_other_flag(L, name, timing):
    rc, h = _create(L, 8, 5, 2, getattr(cg, name) | timing)
    assert rc == ERR_ARG and h is None and "cgx_create_csr_multi" in _err(L), _err(L)


def test_create_refuses_unknown_bits_and_null_pointers(L):
    rc, h = _create(L, 8, 5, 2, 0x10)
    assert rc == ERR_ARG and h is None
    rc, h = _create(L, 8, 5, 2, HALO_ACTIVE)  # a reported bit is not a creation flag
    assert rc == ERR_ARG and h is None
    arr = (ctypes.c_int * 2)(0, 0)
    assert L.cgx_create_csr_multi(None, 8, 5, 2, arr, 0) == ERR_ARG
    h = ctypes.c_void_p(0xdead)
    assert L.cgx_create_csr_multi(ctypes.byref(h), 8, 5, 2, None, 0) == ERR_ARG and h.value is None


# ---- the Python mirror ------------------------------------------------------------------------------------------
def test_flag_value():
    assert HALO_ACTIVE == 0x20000000


def test_devices_not_with_nrhs_or_precond(built):
    indptr, indices, data = cm.poisson(4)
    with pytest.raises(ValueError, match="devices"):
        cg.Solver.csr(16, 64, devices=[0, 0], nrhs=2)
    with pytest.raises(ValueError, match="devices"):
        cg.Solver.from_csr(indptr, indices, data, devices=[0, 0], nrhs=2)
    with pytest.raises(ValueError, match="devices"):
        cg.Solver.from_csr(indptr, indices, data, devices=[0, 0], precond="jacobi")
    with pytest.raises(ValueError, match="csr_nnz"):
        cg.Solver(16, csr_nnz=64, devices=[0, 0])  # the constructor keeps raising: Solver.csr is the spelling


def test_python_halo_calls_check_before_the_c_call(built):
    indptr, indices, _ = cm.poisson(4)
    with pytest.raises(ValueError, match="indptr\\[n\\]"):
        halo_counts(indptr, indices[:-1], 2)
    with pytest.raises(ValueError, match="outside"):
        halo_list(indptr, indices, 2, 0, 2)
    with pytest.raises(cg.CgxError) as e:
        halo_counts(indptr, indices, 3)
    assert e.value.code == ERR_SHAPE
    with pytest.raises(cg.CgxError) as e:
        halo_counts(indptr, indices, 33)
    assert e.value.code == ERR_ARG
