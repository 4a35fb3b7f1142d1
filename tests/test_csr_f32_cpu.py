"""cgx_set_csr_f32, cgx_spmv_csr_f32 and cgx_spmm_csr_f32 without a GPU: the declarations, the argument checks
that run before any device is touched, the Python keyword's own checks, and the refusals of `cg_hip --csr-a32`."""
import os
import re
import subprocess

import numpy as np
import pytest

import conjugate_gradient_amd as cg

ERR_ARG, ERR_SHAPE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cgx_set_csr_f32", "cgx_spmv_csr_f32", "cgx_spmm_csr_f32")


@pytest.fixture(scope="module")
def L(built):
    return cg.lib()


def _p(a):
    return a.ctypes.data


def _err(L):
    return L.cgx_last_error().decode()


RP = np.array([0, 0, 3, 4, 8], np.int64)
CI = np.array([3, 0, 3, 1, 0, 1, 2, 3], np.int32)
VA32 = np.arange(1, 9, dtype=np.float32)


def test_declared_and_exported(L):
    header = open(os.path.join(ROOT, "include", "cgx.h")).read()
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert "const float *values" in m.group(1), name  # the values are float on every new entry point
        assert getattr(L, name).argtypes is not None, name
    assert "#define CGX_VERSION 101" in header  # new functions only: the version stays
    assert "Float-stored values" in header


def test_set_csr_f32_null_ctx(L):
    assert L.cgx_set_csr_f32(None, _p(RP), _p(CI), _p(VA32)) == ERR_ARG
    assert "cgx_set_csr_f32" in _err(L)


def test_spmv_f32_null_and_shape_checks(L):
    v = np.zeros(16)
    good = [_p(RP), _p(CI), _p(VA32), _p(v), _p(v)]
    for k in range(5):  # every pointer in turn
        args = list(good)
        args[k] = None
        assert L.cgx_spmv_csr_f32(4, 4, *args, None) == ERR_ARG, k
        assert "cgx_spmv_csr_f32" in _err(L)
    for rows, cols in ((-1, 4), (4, -1)):
        assert L.cgx_spmv_csr_f32(rows, cols, *good, None) == ERR_SHAPE
        assert "cgx_spmv_csr_f32" in _err(L)


def test_spmm_f32_null_and_shape_checks(L):
    v = np.zeros(16)
    good = [_p(RP), _p(CI), _p(VA32), 2, _p(v), 4, _p(v), 4]
    for k in (0, 1, 2, 4, 6):  # every pointer in turn
        args = list(good)
        args[k] = None
        assert L.cgx_spmm_csr_f32(4, 4, *args, None) == ERR_ARG, k
        assert "cgx_spmm_csr_f32" in _err(L)
    for nrhs in (0, -1, 9):
        assert L.cgx_spmm_csr_f32(4, 4, _p(RP), _p(CI), _p(VA32), nrhs, _p(v), 4, _p(v), 4, None) == ERR_ARG
        assert "cgx_spmm_csr_f32" in _err(L) and "nrhs" in _err(L)
    for rows, cols, ldv, ldo in ((-1, 4, 4, 4), (4, -1, 4, 4), (4, 4, 3, 4), (4, 4, 4, 3)):
        assert L.cgx_spmm_csr_f32(rows, cols, _p(RP), _p(CI), _p(VA32), 2, _p(v), ldv, _p(v), ldo, None) == ERR_SHAPE
        assert "cgx_spmm_csr_f32" in _err(L)


class _Dev:  # stands in for a DeviceArray: the checks below come before any device is touched
    def __init__(self, count, dtype=np.float64):
        self.count, self.dtype, self.ptr = count, np.dtype(dtype), None


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_a_f32_must_be_a_bool(built, bad):
    va = np.zeros(8)
    V, Out = _Dev(8), _Dev(8)
    with pytest.raises(ValueError, match="a_f32"):
        cg.spmv_csr(RP, CI, va, V, Out, 4, 4, a_f32=bad)
    with pytest.raises(ValueError, match="a_f32"):
        cg.spmm_csr(RP, CI, va, V, Out, 4, 4, 2, a_f32=bad)
    with pytest.raises(ValueError, match="a_f32"):
        cg.Solver.from_csr(RP, CI, va, a_f32=bad)
    with pytest.raises(ValueError, match="a_f32"):  # checked before the solver's own state is looked at
        cg.Solver.set_csr(object(), RP, CI, va, a_f32=bad)


def test_python_checks_with_a_f32_come_before_the_c_call(built):
    va = np.zeros(8)
    V, Out = _Dev(8), _Dev(8)
    with pytest.raises(ValueError, match="rows \\+ 1"):
        cg.spmv_csr(RP[:-1], CI, va, V, Out, 4, 4, a_f32=True)
    with pytest.raises(ValueError, match="8 indices but 7 values"):
        cg.spmv_csr(RP, CI, va[:7], V, Out, 4, 4, a_f32=True)
    with pytest.raises(ValueError, match="float64"):  # the vectors stay double
        cg.spmv_csr(RP, CI, va, _Dev(8, np.float32), Out, 4, 4, a_f32=True)
    with pytest.raises(ValueError, match="nrhs"):
        cg.spmm_csr(RP, CI, va, V, Out, 4, 4, 9, a_f32=True)
    bad = CI.copy()
    bad[5] = -1  # the structure check runs on the host: no device array is ever made
    with pytest.raises(cg.CgxError):
        cg.spmv_csr(RP, bad, va, V, Out, 4, 4, a_f32=True)
    with pytest.raises(cg.CgxError):
        cg.spmm_csr(RP, bad, va, V, Out, 4, 4, 2, a_f32=True)


def test_csr_arrays_round_to_nearest(built):
    data = np.array([1.0 / 3.0, 1.0 + 2.0 ** -24 + 2.0 ** -40, -0.0, 2.0 ** -149, 16777217.0, 0.1, 1.0, 2.0])
    rp, ci, va = cg._csr_arrays(RP, CI, data, True)
    assert va.dtype == np.float32 and np.array_equal(va.view(np.uint32), data.astype(np.float32).view(np.uint32))
    assert va[1] == np.float32(1.0 + 2.0 ** -23) and va[4] == np.float32(16777216.0)  # to nearest, ties to even
    assert cg._csr_arrays(RP, CI, data)[2].dtype == np.float64  # without the keyword: as before


CLI_REFUSED = (["--csr"], ["--fp32-ref"], ["--a-fp32"], ["--symmetric"], ["--gpus", "2"], ["--p2p"], ["--nrhs", "2"],
               ["--spd", "64"])


@pytest.mark.parametrize("extra", CLI_REFUSED, ids=lambda e: e[0])
def test_cli_refusals(built, extra):
    for args in ([*extra, "--csr-a32"], ["--csr-a32", *extra]):
        r = subprocess.run([cg.CLI_PATH, *args, "A.txt", "b.txt", "x0.txt"], capture_output=True, text=True)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "--csr-a32" in r.stderr and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)


def test_cli_names_the_option(built):
    r = subprocess.run([cg.CLI_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--csr-a32" in r.stderr
    # the spelling with two options stays refused
    r = subprocess.run([cg.CLI_PATH, "--csr", "--a-fp32", "A.txt", "b.txt", "x0.txt"], capture_output=True, text=True)
    assert r.returncode == 2
