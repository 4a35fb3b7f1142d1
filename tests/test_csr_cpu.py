"""cgx_create_csr without a GPU: the structure check, the argument checks that run before any device is touched,
and the Python mirror's own checks."""
import ctypes

import numpy as np
import pytest

import conjugate_gradient_amd as cg

# None on a tree without the feature: every test then fails at its first use
CSR_ACTIVE = getattr(cg, "CGX_CSR_ACTIVE", None)

ERR_ARG, ERR_SHAPE, ERR_NODEV = -1, -4, -7
REFUSED = ("CGX_F32_REF", "CGX_A_F32", "CGX_SYMMETRIC", "CGX_HOST_STREAM", "CGX_PHASES", "CGX_COMM_P2P",
           "CGX_NO_OVERLAP", "CGX_DETERMINISTIC")


@pytest.fixture(scope="module")
def L(built):
    return cg.lib()


def _p(a):
    return a.ctypes.data


def _err(L):
    return L.cgx_last_error().decode()


# 4 rows: an empty row, an unsorted row with a duplicate column, a full row
RP = np.array([0, 0, 3, 4, 8], np.int64)
CI = np.array([3, 0, 3, 1, 0, 1, 2, 3], np.int32)


def test_check_accepts_empty_rows_unsorted_columns_and_duplicates(L):
    assert L.cgx_csr_check(4, 8, _p(RP), _p(CI)) == 0
    empty = np.zeros(5, np.int64)
    assert L.cgx_csr_check(4, 0, _p(empty), None) == 0


@pytest.mark.parametrize("rp,ci,nnz,named", [
    ([1, 1, 3, 4, 8], CI, 8, "row_ptr[0] = 1"),
    ([0, 3, 2, 4, 8], CI, 8, "decreases at row 1"),
    ([0, 0, 3, 4, 7], CI, 8, "row_ptr[n] = 7"),
    ([0, 0, 3, 4, 8], [3, 0, 3, 1, 0, -1, 2, 3], 8, "col_idx[5] = -1"),
    ([0, 0, 3, 4, 8], [3, 0, 3, 1, 0, 1, 2, 4], 8, "col_idx[7] = 4"),
])
def test_check_names_the_first_offence(L, rp, ci, nnz, named):
    rp, ci = np.array(rp, np.int64), np.array(ci, np.int32)
    assert L.cgx_csr_check(4, nnz, _p(rp), _p(ci)) == ERR_SHAPE
    assert named in _err(L), _err(L)


def test_check_null_and_sizes(L):
    assert L.cgx_csr_check(4, 8, None, _p(CI)) == ERR_ARG
    assert L.cgx_csr_check(4, 8, _p(RP), None) == ERR_ARG
    assert L.cgx_csr_check(0, 0, _p(RP), _p(CI)) == ERR_ARG
    assert L.cgx_csr_check(4, -1, _p(RP), _p(CI)) == ERR_ARG


def _create(L, n, nnz, flags):
    h = ctypes.c_void_p(0xdead)  # must come back NULL on every refusal
    return L.cgx_create_csr(ctypes.byref(h), n, nnz, 0, flags), h.value


def test_create_refuses_sizes_before_the_device(L):
    for n, nnz in ((0, 5), (-3, 5), (10, -1), (2 ** 31, 5)):
        rc, h = _create(L, n, nnz, cg.CGX_F64)
        assert rc == ERR_ARG and h is None, (n, nnz, rc, h)
        assert "cgx_create_csr" in _err(L)
    assert L.cgx_create_csr(None, 10, 5, 0, 0) == ERR_ARG


@pytest.mark.parametrize("name", REFUSED)
@pytest.mark.parametrize("timing", [0, cg.CGX_TIMING])
def test_create_refuses_every_other_flag_before_the_device(L, name, timing):
    rc, h = _create(L, 10, 5, getattr(cg, name) | timing)
    assert rc == ERR_ARG and h is None
    assert "cgx_create_csr" in _err(L) and name in _err(L), _err(L)


def test_create_unknown_bit(L):
    rc, h = _create(L, 10, 5, 0x10)
    assert rc == ERR_ARG and h is None and "cgx_create_csr" in _err(L)


@pytest.mark.parametrize("flags", [cg.CGX_F64, cg.CGX_TIMING])
def test_accepted_arguments_reach_the_device_check(L, flags):
    rc, h = _create(L, 10, 5, flags)
    if cg.device_count() > 0:  # run where a GPU is visible: the accepted arguments create a context
        assert rc == 0 and h
        assert L.cgx_destroy(h) == 0
    else:
        assert rc == ERR_NODEV and h is None


def test_null_checks(L):
    assert L.cgx_set_csr(None, _p(RP), _p(CI), _p(np.zeros(8))) == ERR_ARG
    v = np.zeros(4)
    for args in ((None, _p(CI), _p(v), _p(v), _p(v)), (_p(RP), None, _p(v), _p(v), _p(v)),
                 (_p(RP), _p(CI), None, _p(v), _p(v)), (_p(RP), _p(CI), _p(v), None, _p(v)),
                 (_p(RP), _p(CI), _p(v), _p(v), None)):
        assert L.cgx_spmv_csr(4, 4, *args, None) == ERR_ARG
    assert L.cgx_spmv_csr(-1, 4, _p(RP), _p(CI), _p(v), _p(v), _p(v), None) == ERR_SHAPE


def test_flag_value():
    assert CSR_ACTIVE == 0x8000000


@pytest.mark.parametrize("kw", [dict(devices=[0]), dict(rank=0, nranks=1, unique_id=b"\0" * 128), dict(poisson_m=4),
                                dict(nrhs=2)])
def test_solver_csr_not_with_other_modes(built, kw):
    with pytest.raises(ValueError, match="csr_nnz"):
        cg.Solver(16, csr_nnz=10, **kw)
    with pytest.raises(ValueError, match="csr_nnz"):
        cg.Solver(16, csr_nnz=-1)


def _bare(n, nnz):
    s = cg.Solver.__new__(cg.Solver)  # no context: the shape checks come before the C call
    s.n, s.csr_nnz, s._h, s.nrhs = n, nnz, None, None
    return s


def test_set_csr_shape_errors_before_the_c_call(built):
    s = _bare(4, 8)
    va = np.zeros(8)
    with pytest.raises(ValueError, match="n \\+ 1"):
        s.set_csr(RP[:-1], CI, va)
    with pytest.raises(ValueError, match="8 indices but 7 values"):
        s.set_csr(RP, CI, va[:7])
    with pytest.raises(ValueError, match="room for 7"):
        _bare(4, 7).set_csr(RP, CI, va)
    with pytest.raises(ValueError, match="csr_nnz"):
        s2 = _bare(4, 8)
        s2.csr_nnz = None
        s2.set_csr(RP, CI, va)

    class M:  # an object with .indptr / .indices / .data is accepted
        indptr, indices, data = RP[:-1], CI, va
    with pytest.raises(ValueError, match="n \\+ 1"):
        s.set_csr(M)
