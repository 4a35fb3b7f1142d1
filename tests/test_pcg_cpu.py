"""Diagonal preconditioning of CSR contexts, the parts that need no GPU: the host-only check of a caller's
diagonal, the NULL refusals of the four context entry points, `cg_hip --jacobi`'s option check (which runs before any
device is touched), and the CPU reference itself (tests/_pcg_ref.py) against its own table and np.linalg.solve."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _pcg_ref as pr
import conjugate_gradient_amd as cg
import oracle

ERR_ARG, ERR_SHAPE = -1, -4


def diag_check(n, arr):
    L = cg.lib()
    rc = L.cgx_precond_diag_check(n, None if arr is None else arr.ctypes.data)
    return rc, L.cgx_last_error().decode()


def test_constants_match_header():
    """The kinds by name (the CGX_* names of the package are its flag words, test_flag_constants_match_header's;
    a kind is not a bit of one) and the reported flag bit."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgx.h")) as f:
        hdr = dict((m.group(1), int(m.group(2), 0)) for m in re.finditer(r"#define\s+(CGX_\w+)\s+(0x[0-9a-fA-F]+|\d+)", f.read()))
    assert cg.PRECOND_KINDS == {"none": hdr["CGX_PC_NONE"], "jacobi": hdr["CGX_PC_JACOBI"], "diag": hdr["CGX_PC_DIAG"]}
    assert cg.PRECOND_KINDS == {"none": 0, "jacobi": 1, "diag": 2}
    assert cg.CGX_PRECOND_ACTIVE == hdr["CGX_PRECOND_ACTIVE"] == 0x10000000


def test_diag_check_accepts_a_positive_vector(built):
    v = np.array([1.0, 0.25, 5e-324, 1.7e308, 3.0])
    assert diag_check(v.size, v)[0] == 0
    assert diag_check(1, np.array([2.0]))[0] == 0


@pytest.mark.parametrize("bad,shown", [(0.0, "0"), (-2.5, "-2.5"), (np.nan, "nan"), (np.inf, "inf"), (-0.0, "-0")])
def test_diag_check_names_the_first_offence(built, bad, shown):
    v = np.full(9, 0.5)
    v[6] = -1.0  # a later offence: not the one named
    v[4] = bad
    rc, msg = diag_check(v.size, v)
    assert rc == ERR_SHAPE
    assert f"minv[4] = {shown} " in msg, msg


def test_diag_check_refuses_null_and_empty(built):
    assert diag_check(3, None)[0] == ERR_ARG
    assert diag_check(0, np.ones(1))[0] == ERR_ARG
    assert diag_check(-1, np.ones(1))[0] == ERR_ARG


def test_entry_points_refuse_a_null_context(built):
    L = cg.lib()
    k = ctypes.c_int(7)
    buf = np.ones(4)
    assert L.cgx_set_precond(None, cg.PRECOND_KINDS["jacobi"]) == ERR_ARG
    assert L.cgx_set_precond_diag(None, buf.ctypes.data) == ERR_ARG
    assert L.cgx_get_precond(None, ctypes.byref(k)) == ERR_ARG and k.value == 7
    assert L.cgx_get_precond_diag(None, buf.ctypes.data) == ERR_ARG
    assert np.array_equal(buf, np.ones(4))


# what --csr refuses (test_gpu_csr.py::test_cli_csr), and --spd, which takes no matrix file
CSR_REFUSES = (["--fp32-ref"], ["--a-fp32"], ["--symmetric"], ["--gpus", "2"], ["--p2p"], ["--nrhs", "2"])


@pytest.mark.parametrize("extra", [None, *CSR_REFUSES, ["--spd", "64"]], ids=lambda e: "no-csr" if e is None else e[0])
def test_cli_jacobi_needs_a_plain_csr_solve(built, tmp_path, extra):
    """Exit status 2 and one line naming the option, before a file is opened or a device touched: the files named
    here do not exist."""
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    args = ["--jacobi", *paths] if extra is None else ["--csr", "--jacobi", *extra, *paths]
    r = subprocess.run([cg.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and "--jacobi" in lines[0], r.stderr
    assert r.stdout == ""


# ---- the reference against its own table ------------------------------------------------------------------------
def near(got, want, rel):
    return abs(got - want) <= rel * abs(want)


def hold_table(A, b, row, run_plain):
    """The table's row holds: the Jacobi loop count and both margins; the printed ratios to their printed digits
    (6 %) where they are not rounding noise (at >= 1e-3, before <= 1e5); PCG's x against np.linalg.solve; and, where
    it is run, plain CG's loop count (2 %: a count in the thousands moves with the dots' last bits) or its failure
    to converge in 3000 loops."""
    loops, before_t, at_t, plain_t = row
    minv = 1.0 / np.diag(A)
    x, K, before, at = pr.checked_reference(A, b, minv)  # asserts the factor of 3 on both sides
    assert K == loops
    if at_t >= 1e-3:
        assert near(at, at_t, 0.06), (at, at_t)
    if before_t is not None and before_t <= 1e5:
        assert near(before, before_t, 0.06), (before, before_t)
    xs = np.linalg.solve(A, b)
    assert np.linalg.norm(x - xs) <= pr.TOL * np.linalg.norm(xs)
    assert np.linalg.norm(b - A @ x) <= max(pr.TOL * np.linalg.norm(b), pr.EPS)
    if not run_plain:
        return
    if plain_t is None:
        assert pr.pcg(A, b, None, max_iter=3000)[2] == 0
    else:
        _, plain, conv, _ = pr.pcg(A, b, None, max_iter=12000)
        assert conv == 1 and plain >= K
        assert plain == plain_t if plain_t < 100 else near(plain, plain_t, 0.02), (plain, plain_t)


@pytest.mark.parametrize("case", list(pr.MASKED_TABLE), ids=str)
def test_reference_table_masked(built, case):
    n, seed, dec, s = case
    A, b = pr.scale_system(*pr.masked_base(n, seed), dec, s)
    hold_table(A, b, pr.MASKED_TABLE[case], run_plain=n <= 1001)


@pytest.mark.parametrize("case", list(pr.POISSON_TABLE), ids=str)
def test_reference_table_poisson(built, case):
    m, dec, s = case
    A, b = pr.scale_system(oracle.poisson_dense(m), np.ones(m * m), dec, s)
    hold_table(A, b, pr.POISSON_TABLE[case], run_plain=True)


def test_reference_identity_is_plain_cg():
    """minv == 1 is plain CG, and a power of two changes nothing either: the pins the GPU tests put on the kernels
    hold in the reference's own arithmetic."""
    A, b = pr.scale_system(oracle.poisson_dense(7), np.ones(49), 2, 1.0)
    x0, k0, c0, h0 = pr.pcg(A, b, None)
    for c in (1.0, 0.25):
        x, k, cv, h = pr.pcg(A, b, np.full(49, c))
        assert (k, cv) == (k0, c0) and np.array_equal(x, x0) and h == h0
