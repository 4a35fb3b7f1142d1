"""cgx_create_csr_nrhs: several right-hand sides on one CSR matrix (k_csr_mult_f64 at K = 2, 4, 8, cgx_csr_core.h) through every
layer -- the kernel's bits per column against the CPU statement of the SpMV's summation order
(tests/_spmv_order.py) and against cgx_spmv_csr itself, the context's plans, per-column solves against the oracle,
the freeze rule, the host forms, the Poisson matrix and the refusals.

Masked systems are test_gpu_csr.py's: A = oracle.spd_hash(n, seed)[0] with every entry zeroed except where
|i-j| <= 2, or (i+j) % 7 == 0 and |i-j| <= 64, or i % 50 == 0, or j % 50 == 0.  Column j is
s_j * oracle.spd_hash(n, seed + j)[1]; x0 = 0, eps = 1e-10.  The bar is the project's fp64 one per column: the
oracle's loop count, ||x - x_oracle|| <= 1e-10 ||x_oracle||, ||b - A x|| <= max(1e-10 ||b||, 1e-10).

A loop count is asserted only where the oracle alone stands a factor of 3 from the threshold on both sides
(checked_oracle; a condition on the choice of columns, not a tolerance).  Measured on the CPU oracle (ratio
sqrt(r.r) / eps one iteration before the stop / at it):
  (1000, 2), s = (1, 1e-3, 1, 1e-3, 1e-3, 1, 1e-3, 1): 6, 5, 6, 5, 5, 6, 5, 6 loops; before >= 5.96, at <= 0.203
  (2100, 8), s = (1, 2, 1e-3): 6, 6, 5; 8.95 / 0.024, 17.8 / 0.045, 3.46 / 0.0086
  (5, 3), s = (1, 1e-3, 1, 1e-6, 1e-6): 5, 5, 5, 4, 4; before >= 6.35, at <= 0.158
  (130, 5), column index 4 at s = 2 / 1e-3 / 1e-6 / 1e-9: 8 (4.60 / 0.092), 6 (3.52 / 0.089), 4 (3.15 / 0.100),
  2 (4.15 / 0.144)
  Poisson m = 12, b = 1: 21 loops, 362 / 2.4e-6."""
import functools

import numpy as np
import pytest

import _spmv_order as so
import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-10
EPS = 1e-10
# None on a tree without the feature: every test then fails at its first use
spmm_csr = getattr(cg, "spmm_csr", None)
solver_csr = getattr(cg.Solver, "csr", None)
NRHS_ALL = tuple(range(1, 9))
LDV, LDO = 203, 40  # an odd pitch larger than cols; a pitch larger than rows


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
    """(x, loop count) of the oracle from x0 = 0, with the factor-of-3 margin asserted on the oracle alone."""
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


@functools.lru_cache(maxsize=4)
def masked(n, seed):
    """(A masked, dense; its CSR)."""
    A = oracle.spd_hash(n, seed=seed)[0] * mask(n)
    return frozen(A)[0], to_csr(A)


@functools.lru_cache(maxsize=None)
def column(n, seed, j, s):
    """(b, oracle x, oracle loop count) of s * spd_hash(n, seed + j)[1] on the masked A of (n, seed)."""
    b = s * oracle.spd_hash(n, seed=seed + j)[1]
    xo, K = checked_oracle(masked(n, seed)[0], b)
    return frozen(b, xo) + (K,)


SCALES = {(1000, 2): (1.0, 1e-3, 1.0, 1e-3, 1e-3, 1.0, 1e-3, 1.0), (2100, 8): (1.0, 2.0, 1e-3),
          (5, 3): (1.0, 1e-3, 1.0, 1e-6, 1e-6)}
LOOPS = {(1000, 2): [6, 5, 6, 5, 5, 6, 5, 6], (2100, 8): [6, 6, 5], (5, 3): [5, 5, 5, 4, 4]}


def system(n, seed, nrhs):
    """(A, csr, B (nrhs, n), the oracle's x per column, its loop count per column)."""
    A, csr = masked(n, seed)
    cols = [column(n, seed, j, SCALES[n, seed][j]) for j in range(nrhs)]
    return A, csr, np.stack([c[0] for c in cols]), [c[1] for c in cols], [c[2] for c in cols]


def nrhs_solver(csr, B, flags=cg.CGX_F64):
    s = cg.Solver.from_csr(*csr, nrhs=B.shape[0], flags=flags)
    s.set_rows(0, b_rows=B, x_rows=np.zeros(B.shape))
    return s


def meets_bar(x, iters, A, b, xo, K):
    assert iters == K, (iters, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), EPS)


def per_column(s, nrhs):
    return [s.stats_rhs(j) for j in range(nrhs)]


# ---- 1. kernel-level bits: the structure matrix ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def struct_v():
    """Eight columns of standard normals at pitch LDV (the gaps hold NaN: nothing may read them into a sum)."""
    V = np.full(8 * LDV, np.nan)
    rng = np.random.default_rng(4242)
    for j in range(8):
        V[j * LDV:j * LDV + so.STRUCT_COLS] = rng.standard_normal(so.STRUCT_COLS)
    return frozen(V)[0]


def vcol(j):
    return struct_v()[j * LDV:j * LDV + so.STRUCT_COLS]


@functools.lru_cache(maxsize=None)
def struct_expected(T):
    indptr, indices, data, _ = so.structure_matrix()
    return frozen(np.stack([so.spmv_csr(indptr, indices, data, vcol(j), T) for j in range(8)]))[0]


@functools.lru_cache(maxsize=None)
def struct_dense():
    indptr, indices, data, _ = so.structure_matrix()
    dense = np.zeros((so.STRUCT_ROWS, so.STRUCT_COLS))
    np.add.at(dense, (np.repeat(np.arange(so.STRUCT_ROWS), np.diff(indptr)), indices), data)
    return frozen(np.stack([dense @ vcol(j) for j in range(8)]))[0]


def run_spmm(indptr, indices, data, V, rows, cols, nrhs, ldv, ldo):
    """Out as (8, ldo) after one call on an Out pre-filled with NaN."""
    dV = cg.DeviceArray.from_host(V)
    dO = cg.DeviceArray.from_host(np.full(8 * ldo, np.nan))
    spmm_csr(indptr, indices, data, dV, dO, rows, cols, nrhs, ldv=ldv, ldo=ldo)
    out = dO.to_host().reshape(8, ldo)
    dV.free()
    dO.free()
    assert np.isnan(out[:, rows:]).all(), "the kernel stored past the last row"
    assert np.isnan(out[nrhs:]).all(), "the kernel stored a column >= nrhs"
    return out[:nrhs, :rows]


def run_spmv(indptr, indices, data, v, rows, cols):
    dv, dout = cg.DeviceArray.from_host(v), cg.DeviceArray.from_host(np.full(rows, np.nan))
    cg.spmv_csr(indptr, indices, data, dv, dout, rows, cols)
    out = dout.to_host()
    dv.free()
    dout.free()
    return out


@pytest.mark.parametrize("nt", so.POLICIES)
@pytest.mark.parametrize("T", so.TS)
def test_structure_matrix_bits(monkeypatch, T, nt):
    indptr, indices, data, _ = so.structure_matrix()
    want, ref = struct_expected(T), struct_dense()
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt={nt}")
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt={nt}")
    one = np.stack([run_spmv(indptr, indices, data, vcol(j), so.STRUCT_ROWS, so.STRUCT_COLS) for j in range(8)])
    assert same_bits(one, want)  # the one-vector kernel on every column (the contract's other side)
    for nrhs in NRHS_ALL:
        out = run_spmm(indptr, indices, data, struct_v(), so.STRUCT_ROWS, so.STRUCT_COLS, nrhs, LDV, LDO)
        for j in range(nrhs):
            assert same_bits(out[j], want[j]), (T, nt, nrhs, j, np.flatnonzero(out[j] != want[j]))
            assert same_bits(out[j], one[j]), (T, nt, nrhs, j)
            assert np.max(np.abs(out[j] - ref[j])) <= 1e-13 * np.max(np.abs(ref[j]))


@pytest.mark.parametrize("plan", ["T=3,nt=2", "T=8,nt=1", "T=128,nt=8", "T=0"])
def test_plan_string_naming_no_plan_runs_the_default(monkeypatch, plan):
    indptr, indices, data, _ = so.structure_matrix()
    args = (indptr, indices, data, struct_v(), so.STRUCT_ROWS, so.STRUCT_COLS, 3, LDV, LDO)
    monkeypatch.delenv("CGX_SPMM_PLAN", raising=False)
    default = run_spmm(*args)
    assert same_bits(default, struct_expected(8)[:3])  # the kernel-level call's default T
    monkeypatch.setenv("CGX_SPMM_PLAN", plan)
    assert same_bits(run_spmm(*args), default)


# ---- 2. the grid-stride walk -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tridiag_v(n):
    return frozen(np.random.default_rng(7).standard_normal((8, n)))[0]


@pytest.mark.parametrize("nrhs", [3, 8])
@pytest.mark.parametrize("T", [2, 8, 64])
def test_grid_stride_walk(monkeypatch, T, nrhs):
    """70,000 rows under one block per CU: a wave walks several row groups and the last group is partial."""
    n = 70000
    V = tridiag_v(n)
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt=8,bpc=1")
    out = run_spmm(*so.tridiag(n), V.ravel(), n, n, nrhs, n, n)
    for j in range(nrhs):
        want = so.spmv_tridiag(n, V[j], T)
        assert same_bits(out[j], want), (j, np.flatnonzero(out[j] != want)[:8])


# ---- 3. one row, and an empty row ------------------------------------------------------------------------------
@pytest.mark.parametrize("T", so.TS)
def test_one_row(monkeypatch, T):
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt=2")
    V = np.array([-1.25, -1.25])
    out = run_spmm(np.array([0, 1], np.int64), np.array([0], np.int32), np.array([3.0]), V, 1, 1, 2, 1, 1)
    assert same_bits(out, [[-3.75], [-3.75]])
    out = run_spmm(np.array([0, 0], np.int64), np.zeros(0, np.int32), np.zeros(0), V, 1, 1, 2, 1, 1)
    assert same_bits(out, [[0.0], [0.0]])  # an empty row stores +0.0


# ---- 4. Python never launches on unchecked indices ---------------------------------------------------------------
def test_python_never_launches_on_unchecked_indices():
    indptr, indices, data, _ = so.structure_matrix()
    dV, dO = cg.DeviceArray.from_host(struct_v()), cg.DeviceArray.from_host(np.full(8 * LDO, np.nan))
    args = (dV, dO, so.STRUCT_ROWS, so.STRUCT_COLS, 4)
    for bad in (so.STRUCT_COLS, -1):
        idx = indices.copy()
        idx[17] = bad
        with pytest.raises((cg.CgxError, ValueError)):
            spmm_csr(indptr, idx, data, *args, ldv=LDV, ldo=LDO)
    rp = indptr.copy()
    rp[5] = rp[4] - 1
    with pytest.raises(cg.CgxError):
        spmm_csr(rp, indices, data, *args, ldv=LDV, ldo=LDO)
    assert np.isnan(dO.to_host()).all()  # nothing ran


# ---- 5. context plans ------------------------------------------------------------------------------------------
def test_context_plans():
    A, csr, B, XO, KO = system(1000, 2, 3)
    xs = {}
    with nrhs_solver(csr, B) as s:
        info = s.info
        assert info.flags & cg.CGX_CSR_ACTIVE and info.elem_bytes == 8 and info.lda >= 1000
        assert s.nrhs == 3 and s.csr_nnz == int(csr[0][-1])
        for T in so.TS:
            for nt in so.POLICIES:
                s.set_matvec_plan(64 // T, 1, nt)
                pl = s.matvec_plan()
                assert (pl["R"], pl["U"], pl["nt"]) == (64 // T, 1, nt)
                s.set_x(np.zeros((3, 1000)))
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
        assert x2.shape == (3, 1000) and np.isfinite(x2).all()
        assert g2 == g8 and same_bits(x2, x8), T  # the load policy changes no bit
        for j in range(3):
            assert rel(x2[j], xs[2, 2][0][j]) <= 1e-12, (T, j)  # T changes the row sums' rounding only


# ---- 6. solve parity per column ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,nrhs", [(1000, 2, 8), (2100, 8, 3), (5, 3, 5)])
def test_solve_parity_per_column(n, seed, nrhs):
    A, csr, B, XO, KO = system(n, seed, nrhs)
    assert KO == LOOPS[n, seed]  # the oracle's loop counts, as measured
    with nrhs_solver(csr, B) as s:
        X, st = s.solve(eps=EPS)
        per = per_column(s, nrhs)
    assert X.shape == (nrhs, n)
    assert st.iterations == max(KO) and st.converged == 1
    assert st.rr == max(p.rr for p in per)
    for j in range(nrhs):
        assert per[j].converged == 1
        meets_bar(X[j], per[j].iterations, A, B[j], XO[j], KO[j])
    with cg.Solver.from_csr(*csr) as one:  # the one-system context on (A, b_j): the same loop count
        for j in range(nrhs):
            one.set_rows(0, b_rows=B[j], x_rows=np.zeros(n))
            _, s1 = one.solve(eps=EPS)
            assert s1.iterations == KO[j] and s1.converged == 1, (j, s1.iterations, KO[j])


# ---- 7. freeze ----------------------------------------------------------------------------------------------------
def test_freeze():
    n, seed = 130, 5
    A, csr = masked(n, seed)
    c = {s: column(n, seed, 4, s) for s in (2.0, 1e-3, 1e-6, 1e-9)}
    assert [c[s][2] for s in (2.0, 1e-3, 1e-6, 1e-9)] == [8, 6, 4, 2]
    with nrhs_solver(csr, np.stack([c[2.0][0], c[1e-3][0], c[1e-6][0], np.zeros(n)])) as s:
        X, st = s.solve(eps=EPS)
        per = per_column(s, 4)
        s.set_rows(0, b_rows=np.stack([c[1e-9][0], c[1e-3][0], c[1e-6][0], np.zeros(n)]), x_rows=np.zeros((4, n)))
        Y, sty = s.solve(eps=EPS)
        pery = per_column(s, 4)
    assert [p.iterations for p in per] == [8, 6, 4, 1] and [p.converged for p in per] == [1, 1, 1, 1]
    assert st.iterations == 8 and st.converged == 1
    assert [p.iterations for p in pery] == [2, 6, 4, 1] and sty.iterations == 6 and sty.converged == 1
    assert same_bits(X[1], Y[1]) and same_bits(X[2], Y[2])  # frozen columns do not see their neighbours
    assert same_bits(X[3], np.zeros(n)) and same_bits(Y[3], np.zeros(n))  # exactly +0.0
    for j, sc in enumerate((2.0, 1e-3, 1e-6)):
        meets_bar(X[j], per[j].iterations, A, c[sc][0], c[sc][1], c[sc][2])
    meets_bar(Y[0], pery[0].iterations, A, c[1e-9][0], c[1e-9][1], c[1e-9][2])


# ---- 8. independence and determinism ---------------------------------------------------------------------------------
def test_independence_and_determinism(monkeypatch):
    n, seed, nrhs = 1000, 2, 5
    A, csr, B, _, KO = system(n, seed, nrhs)
    perm = [3, 0, 4, 2, 1]
    Z = np.zeros((nrhs, n))
    res = {}
    for gated in (None, "0"):
        if gated is None:
            monkeypatch.delenv("CGX_GATED", raising=False)
        else:
            monkeypatch.setenv("CGX_GATED", gated)
        with nrhs_solver(csr, B) as s:
            X, st = s.solve(Z, eps=EPS)
            its = [p.iterations for p in per_column(s, nrhs)]
            X2, st2 = s.solve(Z, eps=EPS)  # a second solve repeats the first
            assert same_bits(X, X2) and (st2.iterations, st2.converged, st2.rr) == (st.iterations, st.converged, st.rr)
            s.set_x(Z)  # in pieces: every column needs more than 3 iterations
            s.begin()
            assert s.iterate(3) == (3, False)
            done, conv = s.iterate(100, eps=EPS)
            assert (3 + done, conv) == (max(KO), True) and same_bits(s.get_x(), X)
            assert [p.iterations for p in per_column(s, nrhs)] == KO
            s.set_rows(0, b_rows=B[perm], x_rows=Z)
            XP, _ = s.solve(eps=EPS)
            itp = [p.iterations for p in per_column(s, nrhs)]
            xf, stf = s.solve(Z, eps=-1.0, max_iter=9)
        assert its == KO
        assert same_bits(XP, X[perm]) and itp == [KO[p] for p in perm]
        assert stf.iterations == 9 and np.isfinite(xf).all()  # a fixed count past convergence
        res[gated] = (X, its, (st.iterations, st.converged, st.rr))
    assert same_bits(res[None][0], res["0"][0]) and res[None][1:] == res["0"][1:]


# ---- 9. Poisson as CSR, equal columns -----------------------------------------------------------------------------
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


def test_poisson_equal_columns():
    m, n = 12, 144
    b = np.ones(n)
    xo, st = oracle.cg_poisson_f64(m, b, np.zeros(n), eps=EPS)
    K = st.iterations
    before = np.sqrt(oracle.cg_poisson_f64(m, b, np.zeros(n), max_iter=K - 1, eps=-1.0)[1].rr) / EPS
    assert st.converged == 1 and K == 21 and np.sqrt(st.rr) / EPS <= 1 / 3 and before >= 3, (K, before)
    with nrhs_solver(poisson_csr(m), np.ones((4, n))) as s:
        X, sc = s.solve(eps=EPS)
        per = per_column(s, 4)
    assert [p.iterations for p in per] == [21] * 4 and [p.converged for p in per] == [1] * 4
    assert sc.iterations == 21 and sc.converged == 1
    for j in range(4):
        assert same_bits(X[j], X[0]), j
        assert rel(X[j], xo) <= TOL


# ---- 10. lifecycle and refusals on a live context --------------------------------------------------------------------
def test_lifecycle_and_refusals():
    A, csr, B, XO, KO = system(1000, 2, 3)
    Z = np.zeros((3, 1000))
    with solver_csr(1000, int(csr[0][-1]), nrhs=3) as s:
        assert s.nrhs == 3 and s.csr_nnz == int(csr[0][-1])
        for call in (s.begin, lambda: s.solve(eps=EPS), s.residual_norms):
            with pytest.raises(cg.CgxError) as e:  # no matrix yet
                call()
            assert e.value.code == -6
        s.set_csr(*csr)
        s.set_rows(0, b_rows=B, x_rows=Z)
        X1, st1 = s.solve(eps=EPS)
        assert [p.iterations for p in per_column(s, 3)] == KO
        for call in (lambda: s.set_system(A, B), lambda: s.set_rows(0, A_rows=A), s.generate_spd, s.residual_norm,
                     lambda: s.set_precond("jacobi"), lambda: s.set_precond(np.ones(1000))):
            with pytest.raises(cg.CgxError) as e:
                call()
            assert e.value.code == -1
        assert s.precond == "none"
        for bad in (1000, -1):
            idx = csr[1].copy()
            idx[len(idx) // 2] = bad
            with pytest.raises(cg.CgxError) as e:
                s.set_csr(csr[0], idx, csr[2])
            assert e.value.code == -4 and "col_idx" in str(e.value)
        X2, st2 = s.solve(Z, eps=EPS)  # the previous matrix still solves, to the same bits
        assert same_bits(X1, X2) and st2.iterations == st1.iterations == max(KO)
        rn, bn = s.residual_norms()
        for j in range(3):
            nb = np.linalg.norm(B[j])
            assert abs(rn[j] - np.linalg.norm(B[j] - A @ X1[j])) <= 1e-12 * nb
            assert abs(bn[j] - nb) <= 1e-12 * nb
        s.set_csr(csr[0], csr[1], 0.5 * csr[2])  # A / 2 with the same b: x doubles
        s.set_x(Z)
        X4, st4 = s.solve(eps=EPS)
        assert st4.converged == 1
        for j in range(3):
            assert rel(X4[j], 2.0 * XO[j]) <= TOL
            assert np.linalg.norm(B[j] - 0.5 * (A @ X4[j])) <= max(TOL * np.linalg.norm(B[j]), EPS)


def test_timing_flag():
    A, csr, B, XO, KO = system(1000, 2, 3)
    with nrhs_solver(csr, B, flags=cg.CGX_TIMING) as s:
        X, st = s.solve(eps=EPS)
        K = max(KO)
        # one timed SpMM per iteration; the gated loop keeps one iteration in flight past the stop, whose SpMM
        # returns at once but is timed too
        assert st.iterations == K and K <= st.matvec_count <= K + 2 and st.matvec_ms > 0.0
