"""cgx_create_csr: a sparse A in CSR storage (k_csr_mult_f64 at K = 1, cgx_csr_core.h) through every layer -- the
kernel's bits against the CPU statement of its summation order (tests/_spmv_order.py), the context's plans and host
forms, solves against the oracle, the Poisson matrix against the matrix-free operator, the refusals and `cg_hip --csr`.

Masked systems: A = oracle.spd_hash(n, seed)[0] with every entry zeroed except where |i-j| <= 2, or
(i+j) % 7 == 0 and |i-j| <= 64, or i % 50 == 0, or j % 50 == 0 (symmetric; the diagonal keeps A positive definite;
row lengths 32..1000 at n = 1000); b = s * spd_hash(n, seed)[1], x0 = 0, eps = 1e-10.  The bar is the project's fp64
one: the oracle's loop count, ||x - x_oracle|| <= 1e-10 ||x_oracle||, ||b - A x|| <= max(1e-10 ||b||, 1e-10).

The loop count is asserted only where the oracle alone stands a factor of 3 from the threshold on both sides
(checked_oracle, test_gpu_nrhs.py's rule).  Measured on the CPU oracle (ratio sqrt(r.r) / eps one iteration before
the stop / at it): (1, 3, 1): 1 iteration, - / 0; (5, 3, 1): 5, 5.05e5 / 1.4e-7; (130, 5, 1e-9): 2, 4.08 / 0.133;
(1000, 2, 1): 6, 40.2 / 0.186; (1000, 2, 1e-3): 5, 7.9 / 0.040; (2100, 8, 1e-3): 5, 3.26 / 0.009; (5000, 9, 2): 6,
5.58 / 0.009.  Scales that do not keep the factor are not used ((130, 5) at 1, 1e-3, 1e-6; (1000, 2) at 1e-6, 1e-9).
Poisson (b = s everywhere): m = 5, s = 1: 5, 1.3e9 / 1.7e-6; 7, 1: 9, 4.9e7 / 2.0e-6; 12, 1: 21, 362 / 2.4e-6;
16, 2: 32, 3.02 / 0.246 (s = 1 stands at 1.51 / 0.123 and is not used)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _spmv_order as so
import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-10
EPS = 1e-10
# None on a tree without the feature: every test then fails at its first use
spmv_csr = getattr(cg, "spmv_csr", None)
CSR_ACTIVE = getattr(cg, "CGX_CSR_ACTIVE", None)
from_csr = getattr(cg.Solver, "from_csr", None)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def mask(n):
    i, j = np.indices((n, n))
    d = np.abs(i - j)
    return (d <= 2) | (((i + j) % 7 == 0) & (d <= 64)) | (i % 50 == 0) | (j % 50 == 0)


def to_csr(A):
    """(indptr, indices, data) of the entries of A that are not 0, row by row in column order."""
    rows, cols = np.nonzero(A)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))]).astype(np.int64)
    return frozen(indptr, cols.astype(np.int32), np.ascontiguousarray(A[rows, cols]))


def checked_oracle(A, b, margin=3.0):
    """(x, loop count) of the oracle from x0 = 0, with the factor-of-3 margin asserted (test_gpu_nrhs.py's rule)."""
    n = b.size
    xo, st = oracle.cg_f64(A, b, np.zeros(n), eps=EPS)
    K = st.iterations
    at = np.sqrt(st.rr) / EPS
    if K > 1:
        before = np.sqrt(oracle.cg_f64(A, b, np.zeros(n), max_iter=K - 1, eps=-1.0)[1].rr) / EPS
    else:
        before = np.sqrt(b @ b) / EPS
    assert st.converged == 1 and at <= 1.0 / margin and before >= margin, (n, K, before, at)
    return xo, K


@functools.lru_cache(maxsize=2)
def masked(n, seed):
    """(A masked, dense; its CSR; the unscaled b)."""
    A, b = oracle.spd_hash(n, seed=seed)
    A = A * mask(n)
    return frozen(A)[0], to_csr(A), frozen(b)[0]


@functools.lru_cache(maxsize=None)
def system(n, seed, s):
    """(A, csr, b, oracle x, oracle loop count) of the masked system at scale s."""
    A, csr, b0 = masked(n, seed)
    b = frozen(s * b0)[0]
    xo, K = checked_oracle(A, b)
    return A, csr, b, frozen(xo)[0], K


def csr_solver(csr, b, flags=cg.CGX_F64):
    s = from_csr(*csr, flags=flags)
    s.set_rows(0, b_rows=b, x_rows=np.zeros(b.size))
    return s


def meets_bar(x, iters, A, b, xo, K):
    assert iters == K, (iters, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), EPS)


# ---- 1. kernel-level bits: the structure matrix ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def struct_expected(T):
    return so.spmv_csr(*so.structure_matrix(), T)


def run_kernel(indptr, indices, data, v, rows, cols, spare=3):
    dv = cg.DeviceArray.from_host(v)
    dout = cg.DeviceArray.from_host(np.full(rows + spare, np.nan))
    spmv_csr(indptr, indices, data, dv, dout, rows, cols)
    out = dout.to_host()
    dv.free()
    dout.free()
    assert np.isnan(out[rows:]).all(), "the kernel stored past the last row"
    return out[:rows]


@pytest.mark.parametrize("nt", so.POLICIES)
@pytest.mark.parametrize("T", so.TS)
def test_structure_matrix_bits(monkeypatch, T, nt):
    indptr, indices, data, v = so.structure_matrix()
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt={nt}")
    out = run_kernel(indptr, indices, data, v, so.STRUCT_ROWS, so.STRUCT_COLS)
    want = struct_expected(T)
    assert same_bits(out, want), (T, nt, np.flatnonzero(out != want))
    dense = np.zeros((so.STRUCT_ROWS, so.STRUCT_COLS))
    np.add.at(dense, (np.repeat(np.arange(so.STRUCT_ROWS), np.diff(indptr)), indices), data)
    ref = dense @ v
    assert np.max(np.abs(out - ref)) <= 1e-13 * np.max(np.abs(ref))


@pytest.mark.parametrize("plan", ["T=3,nt=2", "T=8,nt=1", "T=128,nt=8", "T=0"])
def test_plan_string_naming_no_plan_runs_the_default(monkeypatch, plan):
    indptr, indices, data, v = so.structure_matrix()
    monkeypatch.delenv("CGX_SPMV_PLAN", raising=False)
    default = run_kernel(indptr, indices, data, v, so.STRUCT_ROWS, so.STRUCT_COLS)
    assert same_bits(default, struct_expected(8))  # the kernel-level call's default T
    monkeypatch.setenv("CGX_SPMV_PLAN", plan)
    assert same_bits(run_kernel(indptr, indices, data, v, so.STRUCT_ROWS, so.STRUCT_COLS), default)


def test_python_never_launches_on_unchecked_indices():
    indptr, indices, data, v = so.structure_matrix()
    dv, dout = cg.DeviceArray.from_host(v), cg.DeviceArray.from_host(np.full(40, np.nan))
    for bad in (so.STRUCT_COLS, -1):
        idx = indices.copy()
        idx[17] = bad
        with pytest.raises((cg.CgxError, ValueError)):
            spmv_csr(indptr, idx, data, dv, dout, so.STRUCT_ROWS, so.STRUCT_COLS)
    rp = indptr.copy()
    rp[5] = rp[4] - 1
    with pytest.raises(cg.CgxError):
        spmv_csr(rp, indices, data, dv, dout, so.STRUCT_ROWS, so.STRUCT_COLS)
    assert np.isnan(dout.to_host()).all()  # nothing ran


# ---- 2. the grid-stride walk -------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 8, 64])
def test_grid_stride_walk(monkeypatch, T):
    """70,000 rows under one block per CU: on 256 CUs a sweep covers 1024 waves x 64 / T rows (32,768 / 8,192 /
    1,024), so a wave walks several groups and the last group is partial."""
    n = 70000
    v = np.random.default_rng(7).standard_normal(n)
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt=8,bpc=1")
    out = run_kernel(*so.tridiag(n), v, n, n)
    want = so.spmv_tridiag(n, v, T)
    assert same_bits(out, want), np.flatnonzero(out != want)[:8]


@pytest.mark.parametrize("T", so.TS)
def test_one_row(monkeypatch, T):
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt=2")
    out = run_kernel(np.array([0, 1], np.int64), np.array([0], np.int32), np.array([3.0]), np.array([-1.25]), 1, 1)
    assert same_bits(out, [-3.75])
    out = run_kernel(np.array([0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0), np.array([-1.25]), 1, 1)
    assert same_bits(out, [0.0])  # an empty row stores +0.0


@pytest.mark.parametrize("n,one_block", [(29, True), (70001, False)])
def test_fused_dot_bits(n, one_block):
    """The fused p.Ap of a context's SpMV against the CPU statement (so.fused_dot), on a one-block grid (29 rows at
    T = 8: four row groups) and on one of more than 256 blocks that wraps (70,001 rows: 8,751 groups).  A context
    does not hand out p.Ap; the first iteration from x0 = 0 shows it: p0 = r0 = b, x1 = alpha b with
    alpha = r0.r0 / p0.Ap0.  b holds signed powers of two, so r0.r0 is exact in any order, b[i] * Ap[i] is exact
    (an FMA onto a sum is one rounded add, as the statement needs) and x1[i] / b[i] is alpha's bits; the matrix
    values are normal, so the sums round and their order shows."""
    T = 8
    rng = np.random.default_rng(n)
    indptr, indices, _ = so.tridiag(n)
    csr = (indptr, indices, rng.standard_normal(indices.size))
    b = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-1, 2, n)
    with csr_solver(csr, b) as s:
        s.set_matvec_plan(64 // T, 1, 2)
        blocks = s.matvec_plan()["blocks"]
        assert (blocks == 1) if one_block else (blocks > 256 and 4 * blocks * (64 // T) < n), blocks
        s.begin()
        assert s.iterate(1, eps=-1.0) == (1, False)
        x = s.get_x()
    pap = so.fused_dot(so.spmv_tridiag(n, b, T, csr), b, T, blocks)
    alpha = float(b @ b) / pap
    print(f"n={n} blocks={blocks} p.Ap={pap!r} alpha={alpha!r} got={x[0] / b[0]!r}")
    assert same_bits(x / b, np.full(n, alpha)), (blocks, alpha, x[0] / b[0])


# ---- 3. context plans ----------------------------------------------------------------------------------------
def test_context_plans():
    A, csr, b, xo, K = system(1000, 2, 1.0)
    xs = {}
    with csr_solver(csr, b) as s:
        flags = s.info.flags
        assert flags & CSR_ACTIVE
        assert not flags & (cg.CGX_FUSED_ACTIVE | cg.CGX_FOLD_ACTIVE | cg.CGX_SMALL_ACTIVE)
        assert s.info.elem_bytes == 8 and s.info.lda >= 1000
        for T in so.TS:
            for nt in so.POLICIES:
                s.set_matvec_plan(64 // T, 1, nt)
                pl = s.matvec_plan()
                assert (pl["R"], pl["U"], pl["nt"]) == (64 // T, 1, nt)
                s.set_x(np.zeros(1000))
                s.begin()
                assert s.iterate(5, eps=-1.0) == (5, False)
                xs[T, nt] = (s.get_x(), pl["blocks"])
        before = s.matvec_plan()
        for R, U, nt in ((8, 2, 8), (3, 1, 8), (64, 1, 8), (8, 1, 0), (8, 1, 1), (0, 1, 8)):
            with pytest.raises(cg.CgxError) as e:
                s.set_matvec_plan(R, U, nt)
            assert e.value.code == -1
            assert s.matvec_plan() == before
    for T in so.TS:
        x2, g2 = xs[T, 2]
        x8, g8 = xs[T, 8]
        assert np.isfinite(x2).all()
        assert g2 == g8 and same_bits(x2, x8), T  # the load policy changes no bit
        assert rel(x2, xs[2, 2][0]) <= 1e-12, T  # T changes the row sums' rounding only


# ---- 4. solve parity against the oracle -------------------------------------------------------------------------
CASES = [(1, 3, 1.0, 1), (5, 3, 1.0, 5), (130, 5, 1e-9, 2), (1000, 2, 1.0, 6), (1000, 2, 1e-3, 5), (2100, 8, 1e-3, 5),
         (5000, 9, 2.0, 6)]


@pytest.mark.parametrize("n,seed,s,loops", CASES)
def test_solve_parity(n, seed, s, loops):
    A, csr, b, xo, K = system(n, seed, s)
    assert K == loops  # the oracle's loop count, as measured
    with csr_solver(csr, b) as sv:
        x, st = sv.solve(eps=EPS)
        assert st.converged == 1
        meets_bar(x, st.iterations, A, b, xo, K)
    with cg.Solver(n) as dense:  # the dense solver on the same masked A: the same loop count
        dense.set_system(A, b)
        xd, sd = dense.solve(eps=EPS)
        assert sd.iterations == K and sd.converged == 1
        assert rel(x, xd) <= TOL


# ---- 5. Poisson as CSR -------------------------------------------------------------------------------------------
def poisson_csr(m):
    """The 5-point matrix of an m x m grid, natural order, columns ascending within a row."""
    k = np.arange(m * m).reshape(m, m)
    ent = [(k[1:, :], k[:-1, :], -1.0), (k[:, 1:], k[:, :-1], -1.0), (k, k, 4.0), (k[:, :-1], k[:, 1:], -1.0),
           (k[:-1, :], k[1:, :], -1.0)]
    rows = np.concatenate([r.ravel() for r, _, _ in ent])
    cols = np.concatenate([c.ravel() for _, c, _ in ent])
    vals = np.concatenate([np.full(r.size, v) for r, _, v in ent])
    order = np.lexsort((cols, rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m * m))]).astype(np.int64)
    return indptr, cols[order].astype(np.int32), vals[order]


@pytest.mark.parametrize("m,s,loops", [(5, 1.0, 5), (7, 1.0, 9), (12, 1.0, 21), (16, 2.0, 32)])
def test_poisson_as_csr(m, s, loops):
    n = m * m
    b = np.full(n, s)
    xo, st = oracle.cg_poisson_f64(m, b, np.zeros(n), eps=EPS)
    K = st.iterations
    before = np.sqrt(oracle.cg_poisson_f64(m, b, np.zeros(n), max_iter=K - 1, eps=-1.0)[1].rr) / EPS
    assert st.converged == 1 and K == loops and np.sqrt(st.rr) / EPS <= 1 / 3 and before >= 3, (K, before)
    indptr, indices, data = poisson_csr(m)
    assert indptr[-1] == 5 * n - 4 * m
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(indptr)), indices] = data
    assert np.array_equal(dense, oracle.poisson_dense(m))
    with csr_solver((indptr, indices, data), b) as sv:
        x, sc = sv.solve(eps=EPS)
    with cg.Solver(None, poisson_m=m) as sp:
        sp.fill(s, 0.0)
        xp, spst = sp.solve(eps=EPS)
    assert sc.iterations == K == spst.iterations and sc.converged == 1
    assert rel(x, xo) <= TOL and rel(x, xp) <= TOL


# ---- 6. host forms --------------------------------------------------------------------------------------------------
def test_host_forms(monkeypatch):
    A, csr, b, xo, K = system(1000, 2, 1.0)
    monkeypatch.delenv("CGX_GATED", raising=False)
    with csr_solver(csr, b) as s:
        x1, st1 = s.solve(x0=np.zeros(1000), eps=EPS)
        assert (st1.iterations, st1.converged) == (K, 1)
        x2, st2 = s.solve(x0=np.zeros(1000), eps=EPS)  # a second solve repeats the first
        assert same_bits(x1, x2) and st2.iterations == K
        assert s.iterate(10, eps=EPS) == (0, True)  # nothing after convergence
        rn, bn = s.residual_norm()
        assert abs(rn - np.linalg.norm(b - A @ x1)) <= 1e-12 * np.linalg.norm(b)
        assert abs(bn - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
        # in pieces
        s.set_x(np.zeros(1000))
        s.begin()
        assert s.iterate(3) == (3, False)
        done, conv = s.iterate(100, eps=EPS)
        assert (3 + done, conv) == (K, True)
        assert same_bits(s.get_x(), x1) and s.stats().iterations == K
        # host-checked convergence
        monkeypatch.setenv("CGX_GATED", "0")
        x3, st3 = s.solve(x0=np.zeros(1000), eps=EPS)
        assert same_bits(x3, x1) and (st3.iterations, st3.converged) == (K, 1)
        monkeypatch.delenv("CGX_GATED")
        # another matrix of no more entries on the same context, then fill
        half = (csr[0], csr[1], 0.5 * csr[2])  # A / 2 with b: x doubles, r.r and the loop count stay
        s.set_csr(*half)
        s.set_x(np.zeros(1000))
        x4, st4 = s.solve(eps=EPS)
        assert st4.converged == 1 and np.linalg.norm(b - 0.5 * (A @ x4)) <= TOL * np.linalg.norm(b)
        assert rel(x4, 2.0 * xo) <= TOL
        s.fill(1.0, 0.0)
        x5, st5 = s.solve(eps=EPS)
        assert st5.converged == 1 and np.linalg.norm(1.0 - 0.5 * (A @ x5)) <= TOL * np.sqrt(1000.0)


def test_timing_flag():
    A, csr, b, xo, K = system(1000, 2, 1.0)
    with csr_solver(csr, b, flags=cg.CGX_TIMING) as s:
        x, st = s.solve(eps=EPS)
        # the gated loop keeps one iteration in flight past the stop: its matVec returns at once but is timed too
        assert st.iterations == K and K <= st.matvec_count <= K + 2 and st.matvec_ms > 0.0


# ---- 7. refusals on a live context ----------------------------------------------------------------------------------
def test_refusals():
    A, csr, b, xo, K = system(1000, 2, 1.0)
    with cg.Solver(1000, csr_nnz=int(csr[0][-1])) as s:
        for call in (s.begin, lambda: s.solve(eps=EPS), s.residual_norm):
            with pytest.raises(cg.CgxError) as e:  # no matrix yet
                call()
            assert e.value.code == -6
        s.set_csr(*csr)
        s.set_rows(0, b_rows=b, x_rows=np.zeros(1000))
        x1, st1 = s.solve(eps=EPS)
        for call, named in ((lambda: s.set_system(A, b), "cgx_set_csr"), (lambda: s.set_rows(0, A_rows=A), "cgx_set_csr"),
                            (s.generate_spd, "cgx_generate_spd")):
            with pytest.raises(cg.CgxError) as e:
                call()
            assert e.value.code == -1 and named in str(e.value)
        for bad in (1000, -1):
            idx = csr[1].copy()
            idx[len(idx) // 2] = bad
            with pytest.raises(cg.CgxError) as e:
                s.set_csr(csr[0], idx, csr[2])
            assert e.value.code == -4 and "col_idx" in str(e.value)
        x2, st2 = s.solve(x0=np.zeros(1000), eps=EPS)  # the previous matrix still solves, to the same bits
        assert same_bits(x1, x2) and st2.iterations == st1.iterations == K


# ---- 8. CLI ----------------------------------------------------------------------------------------------------------
ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")
CLI_B_SCALE = 0.1  # the scale of b at which the oracle's loop count has the margin (checked below)


def test_cli_csr(tmp_path):
    m = 512
    Am, bm = oracle.spd_matlab(m, np.float64)
    Am = Am * mask(m)
    for name, arr, dec in (("A.txt", Am, 4), ("b.txt", CLI_B_SCALE * bm, 9), ("x0.txt", np.zeros(m), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    Aw = cg.read_text(paths[0], m * m, np.float64).reshape(m, m)  # the values the reader reads
    bw = cg.read_text(paths[1], m, np.float64)
    xo, K = checked_oracle(Aw, bw)
    r = subprocess.run([cg.CLI_PATH, "--csr", "--eps", "1e-10", "--print-x", "--stats", *paths], capture_output=True,
                       text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"Computing cg of matrix size : {m * m}"
    assert lines[1].startswith("average clock execution time in seconds: ")
    assert lines[2].startswith(f"iterations: {K} converged: 1"), lines[2]
    assert lines[3] == f"nnz: {np.count_nonzero(Aw)}"
    x = np.array([float(v) for v in lines[-m:]])
    assert len(lines) == 4 + m and rel(x, xo) <= TOL
    for extra in (["--fp32-ref"], ["--a-fp32"], ["--symmetric"], ["--gpus", "2"], ["--p2p"], ["--nrhs", "2"]):
        r = subprocess.run([cg.CLI_PATH, "--csr", *extra, *paths], capture_output=True, text=True, env=ONE_GPU)
        assert r.returncode == 2 and len(r.stderr.strip().splitlines()) == 1, (extra, r.returncode, r.stderr)
