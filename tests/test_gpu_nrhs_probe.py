"""Element-wise probes of the several-right-hand-side CG iteration (cgx_create_nrhs, cgx_create_csr_nrhs): the
K-column vector kernels of csrc/cgx_matvec_nrhs.hip (k_nrhs_residual_f64, k_nrhs_update_r_f64, k_nrhs_update_xp_f64
at K = 2, 4, 8, the per-column reductions of grid_sum_last_block_n) and the start of csrc/cgx_nrhs.hip from x0 != 0.

Every run is three fixed loops (begin, then iterate(1, eps=-1) three times; x read after each, stats_rhs(j).rr after
begin and after each) on rough b, from a rough x0 ("rough": the last column of nrhs >= 2 starts from exactly 0, which
must not trigger the skip of A x0) and from x0 = 0 ("zero"), compared with the same loops in long double
(tests/_nrhs_probe.py, whose docstring holds the systems, the scales S and T and the measured bars):
|x[j][i] - x_ld[j][i]| <= bar S_k[j][i] for every element of every column and |rr_j - rr_ld_j| <= rr_bar T_k[j],
bar = 100 x the spread between fp64 summation orders.  x_1 shows the start kernel's r = b - A x0 row by row, x_2 and
x_3 the r update and the x / p update with the beta from the ring slots.  A neighbour's alpha, a lost odd tail, a wrong
column pitch, a skipped A x0, a beta from the wrong slot or a pad column written back each move some element by at
least 1000 bars (tests/test_nrhs_probe_cpu.py runs those mutations on the CPU).

  a. CSR contexts, every nrhs 1..8, both starts, at the edges of the pair loop (256 pairs per block pass, an odd tail)
     and of the reduction (one block up to 1024 pairs, the hand-off from two blocks on);
  b. dense contexts, every nrhs 1..8, both starts, lda padded and not;
  c. every instantiated plan of the dense and of the CSR matVec, each held to the reference;
  d. the capped grid: more than 2048 * 1024 pairs, the last pair reached by the stride alone;
  e. freeze, element-wise: columns scaled by 2^-40 stop after loop 1 and keep their bits beside running neighbours;
  f. one converged solve from the rough start per context kind.

Beside the bars every run asserts: a second run gives the same bits after every loop (x and r.r), solve(eps=-1,
max_iter=3) the third loop's bits, and cgx_hip_last_error() == 0.  The second run hands x0 over in two row pieces: a
rough x0 after the context was told that x is zero (cgx_fill, or whole rows of zeros), so the pieces have to take the
zero mark back; a zero x0 after a solve, so the start runs its A x0 pass on zeros and has to give the skip's bits.
Each test prints its worst measured ratio to the bar (pytest -s)."""
import numpy as np
import pytest

import _nrhs_probe as nq
import conjugate_gradient_amd as cg
import oracle
from test_gpu_nrhs import PLANS

pytestmark = pytest.mark.gpu
NRHS_ALL = tuple(range(1, nq.MAX_NRHS + 1))
TOL = 1e-10  # this suite's bar on a converged solve
SPMM_TS = (2, 4, 8, 16, 32, 64)
POLICIES = (2, 8)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert getattr(cg.Solver, "csr", None) is not None, "the package has no several-RHS CSR contexts"


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def no_hip_error():
    assert cg.lib().cgx_hip_last_error() == 0


def context(kind, n, nrhs):
    """A context of the kind with its matrix set (b = 0, x = 0)."""
    op = nq.operator(kind, n)
    if kind == "csr":
        return cg.Solver.from_csr(*op.csr(), nrhs=nrhs)
    s = cg.Solver(n, nrhs=nrhs)
    try:
        s.set_system(op.dense(), np.zeros((nrhs, n)))
    except Exception:
        s.close()
        raise
    return s


def snapshots(s, nrhs, eps=-1.0):
    """(x after each of the loops 1, 2, 3; r.r per column after begin and after each loop) from the context's b, x."""
    s.begin()
    xs, rrs = [], [[s.stats_rhs(j).rr for j in range(nrhs)]]
    for _ in nq.KS:
        assert s.iterate(1, eps=eps) == (1, False)
        xs.append(s.get_x())
        rrs.append([s.stats_rhs(j).rr for j in range(nrhs)])
    return xs, np.array(rrs)


def in_pieces(s, B, X0, mark):
    """x0 again, in two row pieces.  mark "fill" / "rows": the context is first told that every x is zero (cgx_fill,
    or whole rows of zeros), so a rough piece has to take the zero mark back.  mark None: the pieces follow a solve,
    whose x is not zero; pieces of zeros then leave the start on its A x0 pass, which has to give the skip's bits."""
    n = X0.shape[1]
    if mark == "fill":
        s.fill(0.0, 0.0)
        s.set_rows(0, b_rows=B)
    elif mark == "rows":
        s.set_rows(0, x_rows=np.zeros(X0.shape))
    h = n // 2
    if h:
        s.set_rows(0, x_rows=np.ascontiguousarray(X0[:, :h]))
    s.set_rows(h, x_rows=np.ascontiguousarray(X0[:, h:]))


def held_to_reference(cols, refs, xs, rrs, what):
    """The worst ratio to the bar of x and of r.r; raises on any element beyond its bar."""
    nrhs, n = len(cols), cols[0].n
    worst_x, worst_rr, bad = 0.0, 0.0, []
    for j, (c, ref) in enumerate(zip(cols, refs)):
        for k, x in zip(nq.KS, xs):
            q = nq.ratios(x[j], ref.X[k], ref.S[k]) / nq.bar(c, k)
            worst_x = max(worst_x, float(np.max(q)))
            if not np.all(q <= 1.0):  # NaN included
                rows = np.flatnonzero(~(q <= 1.0))
                bad.append(("x", j, k, rows.size, [(int(i), float(q[i])) for i in rows[:8]]))
        for k in nq.rr_loops(n):
            q = float(abs(nq.LD(rrs[k][j]) - ref.RR[k]) / ref.T[k]) / nq.rr_bar(c, k)
            worst_rr = max(worst_rr, q)
            if not q <= 1.0:
                bad.append(("rr", j, k, q))
    assert not bad, (what, "x: column, loop, elements beyond the bar, the first (row, ratio); rr: column, loop, ratio",
                     bad)
    assert len(xs) == len(nq.KS) and xs[0].shape == (nrhs, n)
    return worst_x, worst_rr


def probe(s, kind, n, nrhs, variant, what, by_fill=False):
    """The probe of one case on the context s (its matrix set): every element of every column after every loop and
    r.r to their bars, then the bits of a second run and of the one-call form.  Returns the worst ratios."""
    cols = nq.columns(kind, n, nrhs, variant)
    refs = nq.references(cols)
    B, X0 = nq.rhs(cols)
    s.set_rows(0, b_rows=B, x_rows=X0)
    xs, rrs = snapshots(s, nrhs)
    worst = held_to_reference(cols, refs, xs, rrs, (what, variant, nrhs))
    in_pieces(s, B, X0, None if variant == "zero" else "fill" if by_fill else "rows")
    again, rrs_again = snapshots(s, nrhs)
    assert all(same_bits(a, x) for a, x in zip(again, xs)) and same_bits(rrs_again, rrs), (what, variant, nrhs)
    x3, st = s.solve(x0=X0, eps=-1.0, max_iter=max(nq.KS))
    assert st.iterations == max(nq.KS) and same_bits(x3, xs[-1]), (what, variant, nrhs)
    assert [s.stats_rhs(j).iterations for j in range(nrhs)] == [max(nq.KS)] * nrhs
    return worst


def report(what, worst):
    wx, wr = (max(w[i] for w in worst) for i in (0, 1))
    print(f"\n[nrhs probe] {what}: x {wx:.3g} of its bar, r.r {wr:.3g} of its bar ({len(worst)} runs)")


def report_x(what, worst):
    print(f"\n[nrhs probe] {what}: x {max(worst):.3g} of its bar")


def every_nrhs(kind, n):
    worst = []
    for nrhs in NRHS_ALL:
        with context(kind, n, nrhs) as s:
            for variant in nq.VARIANTS:
                worst.append(probe(s, kind, n, nrhs, variant, f"{kind} n {n}", by_fill=nrhs % 2 == 0))
    no_hip_error()
    report(f"{kind} n {n}, nrhs 1..8, both starts", worst)


# ---- a. CSR contexts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nq.CSR_SIZES)
def test_csr_probe(n):
    every_nrhs("csr", n)


# ---- b. dense contexts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nq.DENSE_SIZES)
def test_dense_probe(n):
    every_nrhs("dense", n)


# ---- c. every plan ---------------------------------------------------------------------------------------------------
def width(nrhs):
    return 2 if nrhs <= 2 else 4 if nrhs <= 4 else 8


@pytest.mark.parametrize("nrhs", nq.PLAN_DENSE[1])
def test_dense_probe_every_plan(nrhs):
    """n = 1025: 9 chunks of 128 columns (lda 1152), which no U divides, and one row more than the row groups."""
    n = nq.PLAN_DENSE[0]
    worst = []
    with context("dense", n, nrhs) as s:
        assert s.info.lda % 128 == 0 and s.info.lda // 128 == 9
        for R, U in PLANS[width(nrhs)]:
            for nt in POLICIES:
                s.set_matvec_plan(R, U, nt)
                pl = s.matvec_plan()
                assert (pl["R"], pl["U"], pl["nt"]) == (R, U, nt)
                worst.append(probe(s, "dense", n, nrhs, "rough", f"dense n {n} plan {(R, U, nt)}"))
    no_hip_error()
    assert len(worst) == 2 * len(PLANS[width(nrhs)])
    report(f"dense n {n} nrhs {nrhs}, every plan", worst)


@pytest.mark.parametrize("nrhs", nq.PLAN_CSR[1])
def test_csr_probe_every_plan(nrhs):
    n = nq.PLAN_CSR[0]
    worst = []
    with context("csr", n, nrhs) as s:
        for T in SPMM_TS:
            for nt in POLICIES:
                s.set_matvec_plan(64 // T, 1, nt)
                pl = s.matvec_plan()
                assert (pl["R"], pl["U"], pl["nt"]) == (64 // T, 1, nt)
                worst.append(probe(s, "csr", n, nrhs, "rough", f"csr n {n} T {T} policy {nt}"))
    no_hip_error()
    assert len(worst) == 12
    report(f"csr n {n} nrhs {nrhs}, every plan", worst)


# ---- d. the capped grid -------------------------------------------------------------------------------------------------
def test_csr_probe_capped_grid():
    """n / 2 = 2048 * 1024 + 1 pairs: 2048 blocks, 2048 partials per column, the last pair reached by the stride
    alone, n odd, and nrhs = 3 leaves one pad column."""
    n, nrhs = nq.STRIDE
    assert n // 2 == 2048 * 1024 + 1 and n % 2 == 1 and width(nrhs) - nrhs == 1
    with context("csr", n, nrhs) as s:
        worst = [probe(s, "csr", n, nrhs, "rough", f"csr n {n}")]
    no_hip_error()
    report(f"csr n {n} nrhs {nrhs}, the capped grid", worst)


# ---- e. freeze, element-wise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", nq.FREEZE_SIZES)
def test_freeze_probe(kind, n):
    nq.freeze_conditions(kind, n)  # on the reference alone: a factor of 3 on both sides of FREEZE_EPS
    E, worst = nq.FREEZE_EPS, []
    for pattern, nrhs in nq.FREEZE_PATTERNS:
        what = f"freeze {kind} n {n} {pattern} of {nrhs}"
        cols = nq.columns(kind, n, nrhs, "rough")
        refs = nq.references(cols)
        B, X0 = nq.rhs(cols)
        scaled = nq.scaled_columns(pattern, nrhs)
        f = np.array([nq.FREEZE_SCALE if j in scaled else 1.0 for j in range(nrhs)])
        with context(kind, n, nrhs) as s:
            s.set_rows(0, b_rows=B, x_rows=X0)
            fixed, _ = snapshots(s, nrhs)  # the fixed-count probe of the unscaled columns
            s.set_rows(0, b_rows=B * f[:, None], x_rows=X0 * f[:, None])
            s.begin()
            xs = []
            for k in nq.KS:
                if len(scaled) < nrhs:
                    assert s.iterate(1, eps=E) == (1, False), (what, k)
                elif k == 1:
                    assert s.iterate(1, eps=E) == (1, True), what  # the last column stopped: converged
                else:
                    assert s.iterate(1, eps=E) == (0, True), (what, k)  # a further iterate does nothing
                xs.append(s.get_x())
            per = [s.stats_rhs(j) for j in range(nrhs)]
        for j in range(nrhs):
            if j in scaled:
                assert (per[j].iterations, per[j].converged) == (1, 1), (what, j)
                assert same_bits(xs[1][j], xs[0][j]) and same_bits(xs[2][j], xs[0][j]), (what, j)
                assert same_bits(xs[0][j], fixed[0][j] * nq.FREEZE_SCALE), (what, j)  # exact: a power of two
            else:
                assert (per[j].iterations, per[j].converged) == (3, 0), (what, j)
                assert all(same_bits(xs[k][j], fixed[k][j]) for k in range(3)), (what, j)
        # to the reference: a frozen column's x_1 after every loop, a running column's x_k
        for j, (c, ref) in enumerate(zip(cols, refs)):
            for k, x in zip(nq.KS, xs):
                at = 1 if j in scaled else k
                q = nq.ratios(x[j], ref.X[at] * nq.LD(f[j]), ref.S[at] * f[j]) / nq.bar(c, at)
                assert np.all(q <= 1.0), (what, j, k, float(np.max(q)))
                worst.append(float(np.max(q)))
    no_hip_error()
    report_x(f"freeze {kind} n {n}, {len(nq.FREEZE_PATTERNS)} patterns", worst)


# ---- f. one converged solve from the rough start -------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", nq.FREEZE_SIZES)
def test_converged_solve_from_the_rough_start(kind, n):
    nrhs, eps = 8, 1e-10
    A = nq.operator(kind, n).dense()
    B, X0 = nq.rhs(nq.columns(kind, n, nrhs, "rough"))
    with context(kind, n, nrhs) as s:
        s.set_rows(0, b_rows=B)
        X, st = s.solve(x0=X0, eps=eps)
        per = [s.stats_rhs(j) for j in range(nrhs)]
    no_hip_error()
    assert st.converged == 1 and all(p.converged == 1 for p in per)
    worst = 0.0
    for j in range(nrhs):
        xo, so = oracle.cg_f64(A, B[j], X0[j].copy(), eps=eps)
        assert so.converged == 1
        assert np.linalg.norm(B[j] - A @ X[j]) <= max(TOL * np.linalg.norm(B[j]), eps), j
        d = np.linalg.norm(X[j] - xo) / np.linalg.norm(xo)
        assert d <= TOL, (j, d)
        worst = max(worst, d)
    print(f"\n[nrhs probe] converged {kind} n {n} nrhs {nrhs}: ||x - x_oracle|| / ||x_oracle|| <= {worst:.3g}")
