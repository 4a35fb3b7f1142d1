"""cgx_create_csr_nrhs and cgx_spmm_csr without a GPU: the argument checks that run before any device is touched,
the kernel-level call's NULL and shape checks, the Python mirror's own checks, and the declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

import conjugate_gradient_amd as cg

# None on a tree without the feature: every test then fails at its first use
spmm_csr = getattr(cg, "spmm_csr", None)
solver_csr = getattr(cg.Solver, "csr", None)

ERR_ARG, ERR_SHAPE, ERR_NODEV = -1, -4, -7
REFUSED = ("CGX_F32_REF", "CGX_A_F32", "CGX_SYMMETRIC", "CGX_HOST_STREAM", "CGX_PHASES", "CGX_COMM_P2P",
           "CGX_NO_OVERLAP", "CGX_DETERMINISTIC")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(built):
    return cg.lib()


def _p(a):
    return a.ctypes.data


def _err(L):
    return L.cgx_last_error().decode()


RP = np.array([0, 0, 3, 4, 8], np.int64)
CI = np.array([3, 0, 3, 1, 0, 1, 2, 3], np.int32)


def _create(L, n, nnz, nrhs, flags):
    h = ctypes.c_void_p(0xdead)  # must come back NULL on every refusal
    return L.cgx_create_csr_nrhs(ctypes.byref(h), n, nnz, nrhs, 0, flags), h.value


@pytest.mark.parametrize("n,nnz,nrhs,named", [(0, 5, 2, "n must be"), (-3, 5, 2, "n must be"), (10, -1, 2, "nnz must be"),
                                              (2 ** 31, 5, 2, "2^31"), (10, 5, 0, "nrhs must be"),
                                              (10, 5, -1, "nrhs must be"), (10, 5, 9, "nrhs must be")])
def test_create_refuses_sizes_before_the_device(L, n, nnz, nrhs, named):
    rc, h = _create(L, n, nnz, nrhs, cg.CGX_F64)
    assert rc == ERR_ARG and h is None, (rc, h)
    assert "cgx_create_csr_nrhs" in _err(L) and named in _err(L), _err(L)


def test_create_null_ctx(L):
    assert L.cgx_create_csr_nrhs(None, 10, 5, 2, 0, 0) == ERR_ARG
    assert "cgx_create_csr_nrhs" in _err(L)


@pytest.mark.parametrize("name", REFUSED)
@pytest.mark.parametrize("timing", [0, cg.CGX_TIMING])
def test_create_refuses_every_other_flag_before_the_device(L, name, timing):
    rc, h = _create(L, 10, 5, 3, getattr(cg, name) | timing)
    assert rc == ERR_ARG and h is None
    assert "cgx_create_csr_nrhs" in _err(L) and name in _err(L), _err(L)


def test_create_unknown_bit(L):
    rc, h = _create(L, 10, 5, 3, 0x10)
    assert rc == ERR_ARG and h is None and "cgx_create_csr_nrhs" in _err(L)


@pytest.mark.parametrize("nrhs", [1, 2, 5, 8])
@pytest.mark.parametrize("flags", [cg.CGX_F64, cg.CGX_TIMING])
def test_accepted_arguments_reach_the_device_check(L, flags, nrhs):
    rc, h = _create(L, 10, 5, nrhs, flags)
    if cg.device_count() > 0:  # run where a GPU is visible: the accepted arguments create a context
        assert rc == 0 and h
        assert L.cgx_destroy(h) == 0
    else:
        assert rc == ERR_NODEV and h is None


def test_spmm_null_and_shape_checks(L):
    v = np.zeros(16)
    good = [_p(RP), _p(CI), _p(v), 2, _p(v), 4, _p(v), 4]
    for k in (0, 1, 2, 4, 6):  # every pointer in turn
        args = list(good)
        args[k] = None
        assert L.cgx_spmm_csr(4, 4, *args, None) == ERR_ARG, k
        assert "cgx_spmm_csr" in _err(L)
    for nrhs in (0, -1, 9):
        assert L.cgx_spmm_csr(4, 4, _p(RP), _p(CI), _p(v), nrhs, _p(v), 4, _p(v), 4, None) == ERR_ARG
        assert "nrhs" in _err(L)
    for rows, cols, ldv, ldo in ((-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, 3, 4), (4, 4, 4, 3)):
        assert L.cgx_spmm_csr(rows, cols, _p(RP), _p(CI), _p(v), 2, _p(v), ldv, _p(v), ldo, None) == ERR_SHAPE
        assert "cgx_spmm_csr" in _err(L)


class _Dev:  # stands in for a DeviceArray: the checks below come before any device is touched
    def __init__(self, count, dtype=np.float64):
        self.count, self.dtype, self.ptr = count, np.dtype(dtype), None


def test_python_spmm_checks_come_before_the_c_call(built):
    va = np.zeros(8)
    V, Out = _Dev(8), _Dev(8)
    for nrhs in (0, 9, 2.0):
        with pytest.raises(ValueError, match="nrhs"):
            spmm_csr(RP, CI, va, V, Out, 4, 4, nrhs)
    with pytest.raises(ValueError, match="rows \\+ 1"):
        spmm_csr(RP[:-1], CI, va, V, Out, 4, 4, 2)
    with pytest.raises(ValueError, match="8 indices but 7 values"):
        spmm_csr(RP, CI, va[:7], V, Out, 4, 4, 2)
    with pytest.raises(ValueError, match="ldv >= cols"):
        spmm_csr(RP, CI, va, V, Out, 4, 4, 2, ldv=3)
    with pytest.raises(ValueError, match="ldo >= rows"):
        spmm_csr(RP, CI, va, V, Out, 4, 4, 2, ldo=3)
    with pytest.raises(ValueError, match="spmm_csr V"):
        spmm_csr(RP, CI, va, _Dev(7), Out, 4, 4, 2)
    with pytest.raises(ValueError, match="spmm_csr Out"):
        spmm_csr(RP, CI, va, V, _Dev(8), 4, 4, 2, ldo=5)
    with pytest.raises(ValueError, match="float64"):
        spmm_csr(RP, CI, va, _Dev(8, np.float32), Out, 4, 4, 2)
    # the structure check runs on the host: a bad index raises with no device array ever made
    bad = CI.copy()
    bad[5] = 4
    with pytest.raises((cg.CgxError, ValueError)):
        spmm_csr(RP, bad, va, V, Out, 4, 4, 2)
    bad[5] = -1
    with pytest.raises(cg.CgxError):
        spmm_csr(RP, bad, va, V, Out, 4, 4, 2)


def test_solver_spellings(built):
    with pytest.raises(ValueError, match="csr_nnz"):  # the constructor keeps refusing the pair
        cg.Solver(16, csr_nnz=10, nrhs=2)
    for nrhs in (0, 9, 2.5):
        with pytest.raises(ValueError, match="nrhs"):
            solver_csr(16, 10, nrhs=nrhs)
    with pytest.raises(ValueError, match="nnz"):
        solver_csr(16, -1, nrhs=2)
    with pytest.raises(ValueError, match="n must"):
        solver_csr(0, 5, nrhs=2)
    with pytest.raises(ValueError, match="preconditioner"):
        cg.Solver.from_csr(RP, CI, np.zeros(8), nrhs=2, precond="jacobi")
    if cg.device_count() == 0:  # accepted arguments reach the C call, which finds no device
        with pytest.raises(cg.CgxError) as e:
            solver_csr(16, 10, nrhs=2)
        assert e.value.code == ERR_NODEV


def test_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "cgx.h")).read()
    for name in ("cgx_create_csr_nrhs", "cgx_spmm_csr"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name).argtypes is not None, name
    assert "spmm_csr" in cg.__all__
    assert "#define CGX_VERSION 101" in header
