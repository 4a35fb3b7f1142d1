"""cgx_set_precond: Jacobi and caller-supplied diagonal preconditioning of cgx_create_csr contexts (cgx_pcg.hip),
through every layer -- the extracted diagonal's bits, the refusals, the kernels' bit-level pins against plain CG,
solves against the CPU reference (tests/_pcg_ref.py, whose docstring holds the systems and the measured margins), the
host forms, the lifecycle and `cg_hip --csr --jacobi`.

The bar is the project's fp64 one: the reference's loop count (asserted where the reference alone stands a factor of
3 from the threshold on both sides, which every case of the table does), ||x - x_ref|| <= 1e-10 ||x_ref||,
||b - A x|| <= max(1e-10 ||b||, 1e-10)."""
import os
import subprocess

import numpy as np
import pytest

import _pcg_ref as pr
import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
EPS, TOL = pr.EPS, pr.TOL
ERR_ARG, ERR_SHAPE, ERR_STATE = -1, -4, -6
# None on a tree without the feature: every test then fails at its first use
from_csr = getattr(cg.Solver, "from_csr", None)
PRECOND_ACTIVE = getattr(cg, "CGX_PRECOND_ACTIVE", None)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def bits(v):
    return np.float64(v).view(np.uint64)


def csr_solver(csr, b, precond=None):
    s = from_csr(*csr, precond=precond)
    s.set_rows(0, b_rows=b, x_rows=np.zeros(b.size))
    return s


def no_hip_error():
    assert cg.lib().cgx_hip_last_error() == 0


# ---- 1. the extracted diagonal's bits ---------------------------------------------------------------------------
def hand_made():
    """6 rows, columns unsorted, row 2's diagonal stored three times: 0.1 + 0.2 + 0.3 in stored order is
    0.6000000000000001, in the reverse order 0.6."""
    rows = [([3, 0], [0.5, 4.0]), ([1, 5, 0], [3.0, -0.25, 0.5]), ([2, 4, 2, 0, 2], [0.1, 1.0, 0.2, -0.5, 0.3]),
            ([5, 3, 0], [0.125, 7.0, 0.5]), ([2, 4], [1.0, 2.5]), ([3, 1, 5], [0.125, -0.25, 1.5])]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32)
    data = np.concatenate([v for _, v in rows]).astype(np.float64)
    diag = np.array([4.0, 3.0, (0.0 + 0.1 + 0.2) + 0.3, 7.0, 2.5, 1.5])
    assert diag[2] != (0.0 + 0.3 + 0.2) + 0.1
    return (indptr, indices, data), diag


def test_jacobi_diagonal_bits():
    A, csr, b, minv, xo, K = pr.masked_system(1000, 2, 6, 1.0)
    with csr_solver(csr, b) as s:
        assert s.precond == "none" and not s.info.flags & PRECOND_ACTIVE
        s.set_precond("jacobi")
        assert s.precond == "jacobi" and s.info.flags & PRECOND_ACTIVE
        assert same_bits(s.precond_diag(), 1.0 / np.diag(A))
    csr6, diag = hand_made()
    with from_csr(*csr6, precond="jacobi") as s:
        assert same_bits(s.precond_diag(), 1.0 / diag)
    no_hip_error()


# ---- 2. refused diagonals -----------------------------------------------------------------------------------------
def broken(kind):
    """The 5 x 5 Poisson matrix (n = 25) with the diagonal of rows 17 and 9 spoiled; 9 is the row to name."""
    indptr, indices, data = (a.copy() for a in pr.to_csr(oracle.poisson_dense(5)))
    for row in (17, 9):
        e = indptr[row] + int(np.flatnonzero(indices[indptr[row]:indptr[row + 1]] == row)[0])
        if kind == "missing":
            indices, data = np.delete(indices, e), np.delete(data, e)
            indptr[row + 1:] -= 1
        else:
            data[e] = {"zero": 0.0, "negative": -4.0, "nan": np.nan}[kind]
    return indptr, indices, data


@pytest.mark.parametrize("kind", ["missing", "zero", "negative", "nan"])
def test_refused_diagonals(kind):
    csr = broken(kind)
    with csr_solver(csr, np.ones(25)) as s:
        x_before, st_before = s.solve(x0=np.zeros(25), eps=-1.0, max_iter=3)
        for state in ("none", "diag"):
            if state == "diag":
                s.set_precond(np.full(25, 0.5))
            with pytest.raises(cg.CgxError) as e:
                s.set_precond("jacobi")
            assert e.value.code == ERR_SHAPE and "row 9 " in str(e.value), str(e.value)
            assert s.precond == state
            if state == "diag":
                assert same_bits(s.precond_diag(), np.full(25, 0.5))
                s.set_precond(None)
            x_after, st_after = s.solve(x0=np.zeros(25), eps=-1.0, max_iter=3)
            assert same_bits(x_after, x_before) and bits(st_after.rr) == bits(st_before.rr)
    no_hip_error()


# ---- 3. identity and power-of-two pins ------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 16])
@pytest.mark.parametrize("n,seed", [(1000, 2), (2101, 8)])
def test_identity_and_power_of_two_are_plain_cg(n, seed, T):
    A, b = pr.masked_base(n, seed)
    with csr_solver(pr.to_csr(A), b) as s:
        s.set_matvec_plan(64 // T, 1, 8)
        runs = {}
        for c in (None, 1.0, 0.25):
            s.set_precond(None if c is None else np.full(n, c))
            assert s.precond == ("none" if c is None else "diag")
            for form, kw in (("converged", dict(eps=EPS)), ("fixed", dict(eps=-1.0, max_iter=12))):
                x, st = s.solve(x0=np.zeros(n), **kw)
                runs[c, form] = (x, st.iterations, st.converged, bits(st.rr))
        assert runs[None, "converged"][2] == 1 and runs[None, "fixed"][1] == 12
        for c in (1.0, 0.25):
            for form in ("converged", "fixed"):
                x, it, conv, rr = runs[c, form]
                x0, it0, conv0, rr0 = runs[None, form]
                assert (it, conv) == (it0, conv0), (c, form)
                assert same_bits(x, x0), (c, form, np.flatnonzero(x != x0)[:8])
                assert rr == rr0, (c, form)
    no_hip_error()


# ---- 4. solves -------------------------------------------------------------------------------------------------------
def meets_bar(x, st, A, b, xo, K):
    assert st.converged == 1 and st.iterations == K, (st.iterations, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), EPS)
    assert np.sqrt(st.rr) < EPS  # stats.rr is r.r, the quantity the loop stopped on


@pytest.mark.parametrize("case", list(pr.MASKED_TABLE), ids=str)
def test_solve_masked(case):
    A, csr, b, minv, xo, K = pr.masked_system(*case)
    assert K == pr.MASKED_TABLE[case][0]
    with csr_solver(csr, b, precond="jacobi") as s:
        x, st = s.solve(eps=EPS)
        meets_bar(x, st, A, b, xo, K)
        rn, bn = s.residual_norm()  # the true residual, as on a plain context
        assert abs(rn - np.linalg.norm(b - A @ x)) <= 1e-12 * np.linalg.norm(b)
    no_hip_error()


@pytest.mark.parametrize("case", list(pr.POISSON_TABLE), ids=str)
def test_solve_poisson(case):
    A, csr, b, minv, xo, K = pr.poisson_system(*case)
    assert K == pr.POISSON_TABLE[case][0]
    with csr_solver(csr, b, precond="jacobi") as s:
        meets_bar(*s.solve(eps=EPS), A, b, xo, K)
    with csr_solver(csr, b, precond=minv) as s:  # the same values handed in: the same solve
        assert s.precond == "diag"
        meets_bar(*s.solve(eps=EPS), A, b, xo, K)
    no_hip_error()


# ---- 5. host forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1001, 2, 4, 1.0), (2101, 8, 6, 1.0)], ids=str)
def test_host_forms(monkeypatch, case):
    A, csr, b, minv, xo, K = pr.masked_system(*case)
    n = b.size
    monkeypatch.delenv("CGX_GATED", raising=False)
    with csr_solver(csr, b, precond="jacobi") as s:
        x1, st1 = s.solve(x0=np.zeros(n), eps=EPS)  # device-gated
        meets_bar(x1, st1, A, b, xo, K)
        monkeypatch.setenv("CGX_GATED", "0")  # host-checked
        x2, st2 = s.solve(x0=np.zeros(n), eps=EPS)
        monkeypatch.delenv("CGX_GATED")
        assert same_bits(x2, x1) and (st2.iterations, st2.converged) == (K, 1) and bits(st2.rr) == bits(st1.rr)
        x3, st3 = s.solve(x0=np.zeros(n), eps=-1.0, max_iter=K)  # fixed count
        assert same_bits(x3, x1) and st3.iterations == K and bits(st3.rr) == bits(st1.rr)
        s.set_x(np.zeros(n))  # in pieces
        s.begin()
        assert s.iterate(1) == (1, False) and s.iterate(2) == (2, False)
        done, conv = s.iterate(100, eps=EPS)
        assert (3 + done, conv) == (K, True)
        assert same_bits(s.get_x(), x1) and s.stats().iterations == K
        assert s.iterate(10, eps=EPS) == (0, True)  # nothing after convergence
    no_hip_error()


# ---- 6. the feature matters ------------------------------------------------------------------------------------------
def test_plain_cg_is_not_there_after_the_jacobi_loop_count():
    A, csr, b, minv, xo, K = pr.masked_system(1000, 2, 6, 1.0)
    with csr_solver(csr, b) as s:
        x, st = s.solve(eps=EPS, max_iter=K)
        assert (st.iterations, st.converged) == (K, 0) and np.sqrt(st.rr) > 1e3 * EPS
    no_hip_error()


# ---- 7. lifecycle ----------------------------------------------------------------------------------------------------
def test_lifecycle():
    A, csr, b, minv, xo, K = pr.masked_system(1000, 2, 6, 1.0)
    with cg.Solver(1000, csr_nnz=int(csr[0][-1])) as s:
        for call in (lambda: s.set_precond("jacobi"), lambda: s.set_precond(minv), lambda: s.set_precond(None)):
            with pytest.raises(cg.CgxError) as e:  # no matrix yet
                call()
            assert e.value.code == ERR_STATE
        assert s.precond == "none"
        s.set_csr(*csr)
        s.set_rows(0, b_rows=b, x_rows=np.zeros(1000))
        x_plain, st_plain = s.solve(eps=-1.0, max_iter=9)
        s.set_precond("jacobi")
        xj, stj = s.solve(x0=np.zeros(1000), eps=EPS)
        meets_bar(xj, stj, A, b, xo, K)
        # a second solve with a new b on the same context
        b2 = 0.5 * b[::-1].copy()
        s.set_rows(0, b_rows=b2, x_rows=np.zeros(1000))
        x2, st2 = s.solve(eps=EPS)
        assert st2.converged == 1 and np.linalg.norm(b2 - A @ x2) <= max(TOL * np.linalg.norm(b2), EPS)
        # refusals that change nothing
        for bad in ("ilu", 7):
            with pytest.raises((cg.CgxError, ValueError)):
                s.set_precond(bad)
        assert cg.lib().cgx_set_precond(s._h, cg.PRECOND_KINDS["diag"]) == ERR_ARG
        assert cg.lib().cgx_set_precond(s._h, 3) == ERR_ARG
        for wrong in (np.ones(999), np.ones(1000, np.float32)):
            with pytest.raises(ValueError):
                s.set_precond(wrong)
        worse = minv.copy()
        worse[123] = -1.0
        with pytest.raises(cg.CgxError) as e:
            s.set_precond(worse)
        assert e.value.code == ERR_SHAPE and "minv[123]" in str(e.value)
        assert s.precond == "jacobi" and same_bits(s.precond_diag(), minv)
        # off again: the plain bits are back
        s.set_precond(None)
        assert s.precond == "none" and not s.info.flags & PRECOND_ACTIVE
        with pytest.raises(cg.CgxError) as e:
            s.precond_diag()
        assert e.value.code == ERR_STATE
        s.set_rows(0, b_rows=b, x_rows=np.zeros(1000))
        x_back, st_back = s.solve(eps=-1.0, max_iter=9)
        assert same_bits(x_back, x_plain) and bits(st_back.rr) == bits(st_plain.rr)
        # cgx_set_csr turns preconditioning off
        s.set_precond("jacobi")
        assert s.info.flags & PRECOND_ACTIVE
        s.set_csr(*csr)
        assert s.precond == "none" and not s.info.flags & PRECOND_ACTIVE
        x_again, _ = s.solve(x0=np.zeros(1000), eps=-1.0, max_iter=9)
        assert same_bits(x_again, x_plain)
    no_hip_error()


def test_other_contexts_refuse():
    for make in (lambda: cg.Solver(256), lambda: cg.Solver(256, nrhs=2), lambda: cg.Solver(None, poisson_m=16)):
        with make() as s:
            assert s.precond == "none"
            for call in (lambda: s.set_precond("jacobi"), lambda: s.set_precond(np.ones(s.n)),
                         lambda: s.set_precond(None), s.precond_diag):
                with pytest.raises(cg.CgxError) as e:
                    call()
                assert e.value.code == ERR_ARG
    no_hip_error()


# ---- 8. CLI ----------------------------------------------------------------------------------------------------------
ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")


def test_cli_jacobi(tmp_path):
    n = 130
    A, b = pr.scale_system(*pr.masked_base(n, 5), 3, 1.0)
    for name, arr, dec in (("A.txt", A, 6), ("b.txt", b, 9), ("x0.txt", np.zeros(n), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    Aw = cg.read_text(paths[0], n * n, np.float64).reshape(n, n)  # the matrix as the file holds it
    bw = cg.read_text(paths[1], n, np.float64)
    xo, K, before, at = pr.checked_reference(Aw, bw, 1.0 / np.diag(Aw), require=False)
    r = subprocess.run([cg.CLI_PATH, "--csr", "--jacobi", "--eps", "1e-10", "--print-x", "--stats", *paths],
                       capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"Computing cg of matrix size : {n * n}"
    assert lines[1].startswith("average clock execution time in seconds: ")
    assert lines[2].startswith("iterations: ") and " converged: 1 " in lines[2], lines[2]
    if K is not None:  # the reference keeps the factor of 3 on this file
        assert lines[2].startswith(f"iterations: {K} converged: 1"), (lines[2], K, before, at)
    assert lines[3] == f"nnz: {np.count_nonzero(Aw)}"
    assert lines[4] == "precond: jacobi"
    x = np.array([float(v) for v in lines[-n:]])
    assert len(lines) == 5 + n and rel(x, xo) <= TOL
    assert np.linalg.norm(bw - Aw @ x) <= max(TOL * np.linalg.norm(bw), EPS)
    # a diagonal the library refuses: its message, exit status 1
    Az = A.copy()
    Az[7, 7] = 0.0
    oracle.write_text(paths[0], Az, 6)
    r = subprocess.run([cg.CLI_PATH, "--csr", "--jacobi", *paths], capture_output=True, text=True, timeout=300,
                       env=ONE_GPU)
    assert r.returncode == 1 and "cgx_set_precond" in r.stderr and "row 7 " in r.stderr, (r.returncode, r.stderr)
