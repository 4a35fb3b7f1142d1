"""cgx_set_bsr without a GPU: the block-structure check, the argument checks that run before any device is touched,
the Python mirror's own checks, the constants, and `cg_hip --csr --bsr`'s refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

import conjugate_gradient_amd as cg
from _cases import FIX

ERR_ARG, ERR_SHAPE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# None on a tree without the feature: every test then fails at its first use
BSR_ACTIVE = getattr(cg, "CGX_BSR_ACTIVE", None)
bsr_check = getattr(cg, "bsr_check", None)


@pytest.fixture(scope="module")
def L(built):
    assert hasattr(cg.Solver, "set_bsr"), "the package has no block storage"
    return cg.lib()


def _p(a):
    return a.ctypes.data


def run_cli(*args):
    return subprocess.run([cg.CLI_PATH, *args], capture_output=True, text=True, timeout=120)


def _err(L):
    return L.cgx_last_error().decode()


# 4 block rows: an empty one, an unsorted one with a duplicate block column, a full one
RP = np.array([0, 0, 3, 4, 8], np.int64)
CI = np.array([3, 0, 3, 1, 0, 1, 2, 3], np.int32)


def test_constants_match_the_header():
    with open(os.path.join(ROOT, "include", "cgx.h")) as f:
        src = f.read()
    hdr = dict((m.group(1), int(m.group(2), 0)) for m in re.finditer(r"#define\s+(CGX_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)", src))
    assert hdr["CGX_BSR_ACTIVE"] == 0x40000000 == BSR_ACTIVE
    assert hdr["CGX_MAX_BSR_BLOCK"] == 8 == cg.CGX_MAX_BSR_BLOCK
    assert hdr["CGX_VERSION"] == 101
    bits = [v for k, v in hdr.items() if k.endswith("_ACTIVE") and k != "CGX_BSR_ACTIVE"]
    assert all(v & BSR_ACTIVE == 0 for v in bits)  # a bit of its own


def test_check_accepts_empty_rows_unsorted_columns_and_duplicates(L):
    assert L.cgx_bsr_check(4, 8, _p(RP), _p(CI)) == 0
    assert L.cgx_bsr_check(4, 0, _p(np.zeros(5, np.int64)), None) == 0
    bsr_check(RP, CI)
    bsr_check(RP, CI, 4)


@pytest.mark.parametrize("rp,ci,nnzb,named", [
    ([1, 1, 3, 4, 8], CI, 8, "brow_ptr[0] = 1"),
    ([0, 3, 2, 4, 8], CI, 8, "decreases at block row 1"),
    ([0, 0, 3, 4, 7], CI, 8, "brow_ptr[nb] = 7"),
    ([0, 0, 3, 4, 8], [3, 0, 3, 1, 0, -1, 2, 3], 8, "bcol_idx[5] = -1"),
    ([0, 0, 3, 4, 8], [3, 0, 3, 1, 0, 1, 2, 4], 8, "bcol_idx[7] = 4"),
    ([0, 3, 2, 4, 8], [3, 0, 3, 1, 0, 1, 2, 4], 8, "decreases at block row 1"),  # the first offence, not the last
])
def test_check_names_the_first_offence(L, rp, ci, nnzb, named):
    rp, ci = np.array(rp, np.int64), np.array(ci, np.int32)
    assert L.cgx_bsr_check(4, nnzb, _p(rp), _p(ci)) == ERR_SHAPE
    assert "cgx_bsr_check" in _err(L) and named in _err(L), _err(L)
    if nnzb == ci.size:
        with pytest.raises(cg.CgxError) as e:
            bsr_check(rp, ci)
        assert e.value.code == ERR_SHAPE and named in str(e.value)


def test_check_null_and_sizes(L):
    assert L.cgx_bsr_check(4, 8, None, _p(CI)) == ERR_ARG
    assert L.cgx_bsr_check(4, 8, _p(RP), None) == ERR_ARG
    assert L.cgx_bsr_check(0, 0, _p(RP), _p(CI)) == ERR_ARG
    assert L.cgx_bsr_check(4, -1, _p(RP), _p(CI)) == ERR_ARG
    with pytest.raises(ValueError, match="nb \\+ 1"):
        bsr_check(RP, CI, 5)


def test_csr_check_keeps_its_words(L):
    """The two checks share their rules; cgx_csr_check's messages are the ones it had."""
    rp = np.array([0, 3, 2, 4, 8], np.int64)
    assert L.cgx_csr_check(4, 8, _p(rp), _p(CI)) == ERR_SHAPE
    assert _err(L) == "cgx_csr_check: row_ptr decreases at row 1 (3 -> 2)"
    rp = np.array([0, 0, 3, 4, 7], np.int64)
    assert L.cgx_csr_check(4, 8, _p(rp), _p(CI)) == ERR_SHAPE
    assert _err(L) == "cgx_csr_check: row_ptr[n] = 7, must be nnz = 8"
    assert L.cgx_csr_check(0, 0, _p(RP), _p(CI)) == ERR_ARG
    assert _err(L) == "cgx_csr_check: n must be >= 1 and nnz >= 0"


def test_entry_points_refuse_before_a_device_is_touched(L):
    """No GPU is needed to be refused: a NULL context or pointer, a block size outside [2, 8], a bad shape, a
    misaligned v under an even block size."""
    va = np.zeros(8 * 4)
    assert L.cgx_set_bsr(None, 2, _p(RP), _p(CI), _p(va)) == ERR_ARG and "ctx is NULL" in _err(L)
    v = np.zeros(64)
    ok = (_p(RP), _p(CI), _p(va), _p(v), _p(v))
    for k in range(5):
        args = list(ok)
        args[k] = None
        assert L.cgx_spmv_bsr(4, 4, 2, *args, None) == ERR_ARG and "NULL pointer" in _err(L)
    for bs in (-1, 0, 1, 9):
        assert L.cgx_spmv_bsr(4, 4, bs, *ok, None) == ERR_ARG and "bs must be in [2, 8]" in _err(L)
        assert L.cgx_bsr_tile_values(8, bs, _p(va), _p(va), None) == ERR_ARG and "bs must be in [2, 8]" in _err(L)
    assert L.cgx_spmv_bsr(-1, 4, 2, *ok, None) == ERR_SHAPE
    assert L.cgx_spmv_bsr(4, -1, 2, *ok, None) == ERR_SHAPE
    assert L.cgx_bsr_tile_values(-1, 2, _p(va), _p(va), None) == ERR_SHAPE
    assert L.cgx_bsr_tile_values(8, 2, None, _p(va), None) == ERR_ARG
    assert L.cgx_bsr_tile_values(8, 2, _p(va), None, None) == ERR_ARG
    assert _p(v) % 16 == 0
    assert L.cgx_spmv_bsr(4, 4, 2, _p(RP), _p(CI), _p(va), _p(v) + 8, _p(v), None) == ERR_ARG
    assert "16-byte aligned" in _err(L)


def _bare(n, nnz):
    s = cg.Solver.__new__(cg.Solver)  # no context: the shape checks come before the C call
    s.n, s.csr_nnz, s._h, s.nrhs, s.devices = n, nnz, None, None, None
    return s


def test_set_bsr_shape_errors_before_the_c_call(built):
    s = _bare(8, 32)
    va = np.zeros((8, 2, 2))
    with pytest.raises(ValueError, match="n / bs \\+ 1"):
        s.set_bsr(RP[:-1], CI, va)
    with pytest.raises(ValueError, match="8 indices but 7 blocks"):
        s.set_bsr(RP, CI, va[:7])
    with pytest.raises(ValueError, match="room for 31"):
        _bare(8, 31).set_bsr(RP, CI, va)
    with pytest.raises(ValueError, match="shape \\(nnzb, bs, bs\\)"):
        s.set_bsr(RP, CI, np.zeros(32))
    with pytest.raises(ValueError, match="shape \\(nnzb, bs, bs\\)"):
        s.set_bsr(RP, CI, np.zeros((8, 2, 3)))
    with pytest.raises(ValueError, match="bs = 1 is scalar CSR"):
        s.set_bsr(RP, CI, np.zeros((8, 1, 1)))
    with pytest.raises(ValueError, match="bs must be in \\[2, 8\\]"):
        s.set_bsr(RP, CI, np.zeros((8, 9, 9)))
    with pytest.raises(ValueError, match="real numbers"):
        s.set_bsr(RP, CI, np.zeros((8, 2, 2), np.complex128))
    with pytest.raises(ValueError, match="not divisible by bs = 3"):
        s.set_bsr(RP, CI, np.zeros((8, 3, 3)))
    with pytest.raises(ValueError, match="csr_nnz"):
        s2 = _bare(8, 32)
        s2.csr_nnz = None
        s2.set_bsr(RP, CI, va)
    for attr, val in (("nrhs", 2), ("devices", [0, 0])):
        s3 = _bare(8, 32)
        setattr(s3, attr, val)
        with pytest.raises(ValueError, match="one GPU with one right-hand side"):
            s3.set_bsr(RP, CI, va)

    class M:  # an object with .indptr / .indices / .data, such as scipy's bsr_matrix
        indptr, indices, data = RP[:-1], CI, va
    with pytest.raises(ValueError, match="n / bs \\+ 1"):
        s.set_bsr(M)
    with pytest.raises(ValueError, match="nb \\+ 1 >= 2"):
        cg.Solver.from_bsr(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2, 2)))


def test_spmv_bsr_checks_before_the_c_call(built):
    d = cg.DeviceArray.__new__(cg.DeviceArray)
    d.count, d.dtype, d.ptr = 8, np.dtype(np.float64), None
    va = np.zeros((8, 2, 2))
    with pytest.raises(ValueError, match="nb \\+ 1"):
        cg.spmv_bsr(RP, CI, va, d, d, 3, 4)
    with pytest.raises(ValueError, match="spmv_bsr out"):
        cg.spmv_bsr(np.concatenate([RP, [8]]).astype(np.int64), CI, va, d, d, 5, 4)  # 5 block rows of 2: 10 > 8
    with pytest.raises(ValueError, match="spmv_bsr v"):
        cg.spmv_bsr(RP, CI, va, d, d, 4, 5)
    bad = CI.copy()
    bad[2] = 4  # a block column outside [0, ncolb): refused by the structure check, nothing is uploaded
    with pytest.raises((cg.CgxError, ValueError)):
        cg.spmv_bsr(RP, bad, va, d, d, 4, 4)
    f = cg.DeviceArray.__new__(cg.DeviceArray)
    f.count, f.dtype, f.ptr = 8, np.dtype(np.float32), None
    with pytest.raises(ValueError, match="float64 only"):
        cg.spmv_bsr(RP, CI, va, f, d, 4, 4)


# ---- cg_hip --csr --bsr -------------------------------------------------------------------------------------------
F4 = [os.path.join(FIX, n) for n in ("matrixA1.txt", "vectorb1.txt", "X0.txt")]  # a 4 x 4 system


@pytest.mark.parametrize("val", ["1", "9", "0", "-2", "x", ""])
def test_cli_bsr_block_size(built, val):
    r = run_cli("--csr", "--bsr", val, *F4)
    assert r.returncode == 2 and "--bsr" in r.stderr, r.stdout + r.stderr


def test_cli_bsr_needs_its_value(built):
    r = run_cli("--csr", *F4, "--bsr")
    assert r.returncode == 2 and "--bsr must be an integer in [2, 8]" in r.stderr


def test_cli_bsr_n_not_divisible(built):
    r = run_cli("--csr", "--bsr", "3", *F4)
    assert r.returncode == 2 and "n = 4 is not divisible" in r.stderr, r.stdout + r.stderr
    assert "Computing cg" not in r.stdout  # before anything is read or computed


@pytest.mark.parametrize("extra", [["--csr-a32"], [], ["--fp32-ref", "--csr"], ["--a-fp32", "--csr"],
                                   ["--symmetric", "--csr"], ["--gpus", "2", "--csr"], ["--nrhs", "2", "--csr"],
                                   ["--csr", "--spd", "64"], ["--csr", "--p2p"]])
def test_cli_bsr_refused_combinations(built, extra):
    """--bsr goes with --csr alone: not with --csr-a32, not without --csr, and with nothing --csr is refused with."""
    r = run_cli("--bsr", "2", *extra, *F4)
    assert r.returncode == 2 and ("--bsr" in r.stderr or "--csr" in r.stderr), r.stdout + r.stderr
