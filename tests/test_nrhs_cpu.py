"""cgx_create_nrhs without a GPU: the constant, the C argument checks that run
before any device is touched, and the Python mirror's shape checks that run
before any C call."""
import ctypes

import numpy as np
import pytest

import conjugate_gradient_amd as cg

REFUSED = ["CGX_F32_REF", "CGX_A_F32", "CGX_SYMMETRIC", "CGX_HOST_STREAM", "CGX_PHASES", "CGX_COMM_P2P",
           "CGX_NO_OVERLAP", "CGX_DETERMINISTIC"]


def _bare_solver(n, nrhs):
    s = cg.Solver.__new__(cg.Solver)
    s.n, s.dtype, s.flags, s._h, s.nrhs = n, np.dtype(np.float64), cg.CGX_F64, None, nrhs
    return s


def test_max_nrhs():
    assert cg.CGX_MAX_NRHS == 8


@pytest.mark.parametrize("nrhs", [0, 9, -1])
def test_create_refuses_nrhs_out_of_range(built, nrhs):
    L = cg.lib()
    h = ctypes.c_void_p(1234)
    rc = L.cgx_create_nrhs(ctypes.byref(h), 64, nrhs, 0, cg.CGX_F64)
    assert rc == -1 and h.value is None
    assert b"cgx_create_nrhs" in L.cgx_last_error()


@pytest.mark.parametrize("flag", REFUSED)
def test_create_refuses_every_other_flag(built, flag):
    L = cg.lib()
    for extra in (0, cg.CGX_TIMING):
        h = ctypes.c_void_p(1234)
        rc = L.cgx_create_nrhs(ctypes.byref(h), 64, 2, 0, getattr(cg, flag) | extra)
        assert rc in (-1, -7) and h.value is None
        # the flags are checked before the device: the message names the entry point and the flag
        assert rc == -1 and b"cgx_create_nrhs" in L.cgx_last_error() and flag.encode() in L.cgx_last_error()


def test_create_accepted_flags_reach_the_device_check(built):
    """CGX_F64 and CGX_F64 | CGX_TIMING pass the argument checks: without a GPU the call then fails on the
    device (-7); with one it succeeds."""
    L = cg.lib()
    for flags in (cg.CGX_F64, cg.CGX_TIMING):
        h = ctypes.c_void_p()
        rc = L.cgx_create_nrhs(ctypes.byref(h), 64, 8, 0, flags)
        assert rc in (0, -7), (rc, L.cgx_last_error())
        if rc == 0:
            assert L.cgx_destroy(h) == 0
        else:
            assert h.value is None


def test_matvec_nrhs_argument_checks(built):
    L = cg.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    for nrhs in (0, 9):  # before the pointers are looked at
        assert L.cgx_matvec_nrhs(None, 8, 8, 8, nrhs, None, 8, None, 8, None) == -1
        assert b"nrhs" in L.cgx_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):  # past the nrhs check
        assert L.cgx_matvec_nrhs(args[0], 8, 8, 8, 2, args[1], 8, args[2], 8, None) == -1
        assert b"NULL" in L.cgx_last_error()
    assert L.cgx_matvec_nrhs(p, 4, 8, 8, 2, p, 8, p, 8, None) == -4  # lda < cols


def test_other_entry_points_check_null(built):
    L = cg.lib()
    k = ctypes.c_int(0)
    assert L.cgx_get_nrhs(None, ctypes.byref(k)) == -1
    assert L.cgx_get_stats_rhs(None, 0, ctypes.byref(cg.Stats())) == -1
    assert L.cgx_residual_norms(None, None, None) == -1


def test_python_shape_checks_raise_before_the_c_call():
    n, K = 8, 3
    s = _bare_solver(n, K)  # _h is None: any C call would fail differently
    A = np.eye(n)
    with pytest.raises(ValueError, match=r"b has shape \(8,\), \(3, 8\) needed"):
        s.set_system(A, np.ones(n))
    with pytest.raises(ValueError, match=r"b has shape \(2, 8\)"):  # wrong K
        s.set_system(A, np.ones((2, n)))
    with pytest.raises(ValueError, match=r"b has shape \(3, 9\)"):  # wrong n
        s.set_system(A, np.ones((K, n + 1)))
    with pytest.raises(ValueError, match="x0 has shape"):
        s.set_system(A, np.ones((K, n)), np.zeros(n))
    with pytest.raises(ValueError, match="A has shape"):
        s.set_system(np.eye(n - 1), np.ones((K, n)))
    with pytest.raises(ValueError, match="x has shape"):
        s.set_x(np.zeros(n))
    with pytest.raises(ValueError, match="x0 has shape"):
        s.solve(np.zeros((K + 1, n)))
    with pytest.raises(ValueError, match=r"b_rows has shape \(4,\), \(3, nrows\) needed"):
        s.set_rows(0, None, np.ones(4))
    with pytest.raises(ValueError, match=r"x_rows has shape \(2, 4\)"):
        s.set_rows(0, None, np.ones((K, 4)), np.ones((2, 4)))
    with pytest.raises(ValueError, match="same 4 rows"):
        s.set_rows(0, np.ones((4, n)), np.ones((K, 5)))
    with pytest.raises(ValueError, match="outside"):
        s.set_rows(6, None, np.ones((K, 4)))
    with pytest.raises(ValueError, match="stats_rhs"):
        s.stats_rhs(K)
    # nrhs = 1 still takes (1, n)
    with pytest.raises(ValueError, match=r"\(1, 8\) needed"):
        _bare_solver(n, 1).set_system(A, np.ones(n))


def test_nrhs_does_not_combine_with_other_modes():
    for kw in ({"devices": [0, 0]}, {"rank": 0, "nranks": 1, "unique_id": b"\0" * 128}, {"poisson_m": 4}):
        with pytest.raises(ValueError, match="one GPU"):
            cg.Solver(16, nrhs=2, **kw)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="nrhs must be in"):
            cg.Solver(16, nrhs=bad)


def test_matvec_nrhs_python_checks():
    class Fake:  # stands in for a DeviceArray: the checks run before any pointer is used
        def __init__(self, count, dtype=np.float64):
            self.count, self.dtype, self.ptr = count, np.dtype(dtype), 0
    with pytest.raises(ValueError, match="nrhs must be in"):
        cg.matVec_nrhs(Fake(64), Fake(64), Fake(64), 4, 4, 9)
    with pytest.raises(ValueError, match="matVec_nrhs V"):
        cg.matVec_nrhs(Fake(16), Fake(7), Fake(8), 4, 4, 2)
    with pytest.raises(ValueError, match="matVec_nrhs Out"):
        cg.matVec_nrhs(Fake(16), Fake(8), Fake(7), 4, 4, 2)
    with pytest.raises(ValueError, match="float64 only"):
        cg.matVec_nrhs(Fake(16, np.float32), Fake(8), Fake(8), 4, 4, 2)
