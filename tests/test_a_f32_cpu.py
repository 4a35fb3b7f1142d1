"""CGX_A_F32 without a GPU: the Python mirror's size checks for a float32 A
under the flag, and the library's refusal of flag combinations before any
device is touched."""
import ctypes

import numpy as np
import pytest

import conjugate_gradient_amd as cg


def _bare_solver(n):
    s = cg.Solver.__new__(cg.Solver)
    s.n, s.dtype, s.flags, s._h = n, np.dtype(np.float64), cg.CGX_A_F32, None
    return s


def test_flag_is_a_free_bit():
    assert cg.CGX_A_F32 == 0x2
    others = [v for k, v in vars(cg).items() if k.startswith("CGX_") and k != "CGX_A_F32" and isinstance(v, int)]
    assert all(not v & cg.CGX_A_F32 for v in others)
    assert cg._a_dtype(cg.CGX_A_F32) == np.float32 and cg._dtype(cg.CGX_A_F32) == np.float64
    assert cg._a_dtype(cg.CGX_F64) == np.float64 and cg._a_dtype(cg.CGX_F32_REF) == np.float32


def test_python_mirror_checks_sizes_of_a_float_A():
    s = _bare_solver(8)
    A, b = np.eye(8, dtype=np.float32), np.ones(8)
    with pytest.raises(ValueError, match="A has shape"):
        s.set_system(np.eye(7, dtype=np.float32), b)
    with pytest.raises(ValueError, match="b has shape"):
        s.set_system(A, np.ones(9))
    with pytest.raises(ValueError, match="x0 has shape"):
        s.set_system(A, b, np.zeros(7))
    with pytest.raises(ValueError, match="nrows, >= 8"):
        s.set_rows(0, np.ones((2, 5), np.float32))
    with pytest.raises(ValueError, match="same 2 rows"):
        s.set_rows(0, np.ones((2, 8), np.float32), np.ones(3))
    with pytest.raises(ValueError, match="outside"):
        s.set_rows(7, np.ones((2, 8), np.float32))
    with pytest.raises(ValueError, match="x has shape"):
        s.set_x(np.zeros(3))
    # a float32 A with float64 v / out is the A_F32 matVec; its sizes are checked in the same way
    dA = cg.DeviceArray.__new__(cg.DeviceArray)
    dA.count, dA.dtype, dA.ptr = 15, np.dtype(np.float32), None
    dv = cg.DeviceArray.__new__(cg.DeviceArray)
    dv.count, dv.dtype, dv.ptr = 4, np.dtype(np.float64), None
    with pytest.raises(ValueError, match="matVec A"):
        cg.matVec(dA, dv, dv, rows=4, cols=4)
    with pytest.raises(ValueError, match="matVec v"):
        cg.matVec(dA, dv, dv, rows=3, cols=5)
    d32 = cg.DeviceArray.__new__(cg.DeviceArray)
    d32.count, d32.dtype, d32.ptr = 16, np.dtype(np.float32), None
    with pytest.raises(ValueError, match="one dtype"):  # float64 A with float32 v: no such kernel
        cg.matVec(dv, d32, dv, rows=2, cols=2)


@pytest.mark.parametrize("extra", ["CGX_F32_REF", "CGX_SYMMETRIC", "CGX_HOST_STREAM", "CGX_PHASES"])
def test_refused_flag_combinations_fail_cleanly_without_a_gpu(built, extra):
    """CGX_ERR_ARG (the combination, checked first) or CGX_ERR_NODEV; the
    context pointer stays NULL."""
    L = cg.lib()
    h = ctypes.c_void_p()
    rc = L.cgx_create(ctypes.byref(h), 64, 0, cg.CGX_A_F32 | getattr(cg, extra))
    assert rc in (-1, -7) and not h.value
    if rc == -1:
        assert b"CGX_A_F32" in L.cgx_last_error()
    devs = (ctypes.c_int * 2)(0, 0)
    rc = L.cgx_create_multi(ctypes.byref(h), 64, 2, devs, cg.CGX_A_F32)
    assert rc in (-1, -7) and not h.value
    rc = L.cgx_create_poisson(ctypes.byref(h), 8, 0, cg.CGX_A_F32)
    assert rc in (-1, -7) and not h.value


def test_matvec_dtype_a_f32_only_for_matvec(built):
    """CGX_A_F32 is a dtype of cgx_matvec alone: the vector entry points refuse
    it before touching their pointers."""
    L = cg.lib()
    assert L.cgx_dot(cg.CGX_A_F32, 4, None, None, None, None) == -1
    assert b"CGX_F64 or CGX_F32_REF" in L.cgx_last_error()
    assert L.cgx_matvec(cg.CGX_A_F32, None, 4, 4, 4, None, None, None) == -1  # past the dtype check: NULL pointers
    assert b"NULL" in L.cgx_last_error()
    assert L.cgx_matvec(0x4, None, 4, 4, 4, None, None, None) == -1
    assert b"CGX_A_F32" in L.cgx_last_error()
