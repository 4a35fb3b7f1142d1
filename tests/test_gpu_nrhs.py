"""cgx_create_nrhs: several right-hand sides per pass over A (k_matvec_nrhs_f64
and the K-column iteration of cgx_nrhs.hip).

Systems: A = oracle.spd_hash(n, seed)[0], b_j = s_j * oracle.spd_hash(n, seed + j)[1]
with the scale s_j from SCALES, so the columns stop at different iterations
(the stopping test is absolute).  The bar per column is the project's fp64
one: the oracle's loop count, ||x_j - x_oracle|| <= 1e-10 ||x_oracle||,
||b_j - A x_j|| <= 1e-10 ||b_j||.

The loop-count condition is only safe where sqrt(r.r) / eps is far from 1 at
the stopping iteration and one before it; the bar is a factor of 3 on each
side, and column() asserts it on the oracle alone for every column used.  The
scales in SCALES were chosen from the oracle's ratios (before / at the stop),
e.g. (1000, 2): s = 1: 51 / 0.33, s = 1e-3: 7.9-9.0 / 0.05-0.06, s = 1e-9:
28-30 / 0.19-0.20, while s = 1e-6 gives 1.2-1.4 / 0.008 (too close, not
used); (130, 5): s = 1e-3 gives 1.0-1.25 / 0.02 (not used), s = 1: 15-19 /
0.26-0.33, s = 1e-6: 3.15-3.7 / 0.06, s = 1e-9: 10 / 0.17-0.21; (2100, 8):
s = 1e-6 gives 194-201 / 0.85-0.9 (not used); (8193, 4): only s = 1e-9
(82 / 0.195) keeps the factor of 3."""
import functools
import os
import subprocess

import numpy as np
import pytest

import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-10
EPS = 1e-10
# None on a tree without the feature: every test then fails at its first use
MAX_NRHS = getattr(cg, "CGX_MAX_NRHS", None)
matVec_nrhs = getattr(cg, "matVec_nrhs", None)

# the instantiated (rows per wave, chunks in flight) per width (nrhs rounded up to 2, 4, 8), each with policy 2 and 8
PLANS = {2: [(2, 4), (4, 2), (4, 4), (8, 2)], 4: [(4, 2), (4, 4), (8, 2)], 8: [(4, 1), (4, 2)]}

_A = (1.0, 1e-6, 1e-9, 1.0, 1e-6, 1e-9, 1e-6, 1.0)
SCALES = {  # (n, seed): the scale of column j
    (1, 3): (1.0, 1e-3, 1e-6, 1e-9, 1.0, 1e-3, 1e-6, 1e-9),
    (5, 3): (1.0, 1e-3, 1e-6, 1.0, 1e-6, 1e-3, 1.0, 1e-6),
    (127, 4): _A, (128, 4): _A, (129, 4): _A, (130, 5): _A,
    (257, 4): (1.0, 1e-9, 1.0, 1e-3, 1e-9, 1.0, 1e-9, 1.0),
    (1000, 2): (1.0, 1e-3, 1e-9, 1e-3, 1.0, 1e-9, 1e-3, 1.0),
    (2100, 8): (1.0, 1e-3, 1e-9, 1.0, 1e-3, 1e-9, 1.0, 1e-3),
    (5000, 9): (1.0, 1e-9, 1.0, 1e-9, 1.0, 1e-9, 1.0, 1e-9),
    (8193, 4): (1e-9,) * 8,
}


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=4)
def matrix(n, seed):
    return frozen(oracle.spd_hash(n, seed=seed)[0])[0]


@functools.lru_cache(maxsize=None)
def hash_b(n, seed):
    return frozen(oracle.spd_hash(n, seed=seed)[1])[0]


@functools.lru_cache(maxsize=None)
def scaled_column(n, seed, j, s):
    """(b, oracle x, oracle loop count) of column j at scale s, with the factor-of-3 margin asserted on the oracle:
    sqrt(r.r)/eps >= 3 one iteration before the stop and <= 1/3 at it."""
    b = s * hash_b(n, seed + j)
    xo, K = checked_oracle(matrix(n, seed), b)
    return frozen(b, xo) + (K,)


def checked_oracle(A, b, margin=3.0):
    """(x, loop count) of the oracle from x0 = 0, with the factor-of-3 margin asserted."""
    n = b.size
    xo, so = oracle.cg_f64(A, b, np.zeros(n), eps=EPS)
    K = so.iterations
    at = np.sqrt(so.rr) / EPS
    if K > 1:
        before = np.sqrt(oracle.cg_f64(A, b, np.zeros(n), max_iter=K - 1, eps=-1.0)[1].rr) / EPS
    else:
        before = np.sqrt(b @ b) / EPS
    assert so.converged == 1 and at <= 1.0 / margin and before >= margin, (n, K, before, at)
    return xo, K


def column(n, seed, j):
    return scaled_column(n, seed, j, SCALES[(n, seed)][j])


def system(n, seed, nrhs):
    cols = [column(n, seed, j) for j in range(nrhs)]
    return matrix(n, seed), np.stack([c[0] for c in cols]), [c[1] for c in cols], [c[2] for c in cols]


def meets_bar(x, iters, A, b, xo, K):
    """The residual bar is 1e-10 ||b|| for a column at scale 1 (||b|| > 1 there).  The stopping test is absolute,
    sqrt(r.r) < 1e-10, so a column scaled down to ||b|| < 1 cannot reach 1e-10 ||b|| with any solver -- the
    oracle's own x stands at 2.5e-6 ||b|| on (5, 3) at scale 1e-6 -- and its bar is the stopping rule's own
    bound, ||b - A x|| <= 1e-10: the larger of the two, which is the relative one whenever it can be met."""
    assert iters == K, (iters, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), EPS)


# ---- 1. kernel-level bit parity -----------------------------------------------------------------
SHAPES = [(1, 1, 1), (3, 5, 7), (37, 127, 127), (64, 128, 128), (129, 129, 130), (300, 1000, 1024), (8, 2176, 2176),
          (2048, 4096, 4096)]


def _one_by_one(dA, dV, rows, cols, lda, nrhs, ldv, off):
    """cgx_matvec(CGX_F64) on each column of V where it lies (the same address, so the same alignment)."""
    L = cg.lib()
    out = np.empty((nrhs, rows))
    do = cg.DeviceArray(max(1, rows))
    for j in range(nrhs):
        rc = L.cgx_matvec(cg.CGX_F64, dA.ptr, lda, rows, cols, dV.ptr + 8 * (off + j * ldv), do.ptr, None)
        assert rc == 0, L.cgx_last_error()
        out[j] = do.to_host()[:rows]
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("rows,cols,lda", SHAPES)
def test_kernel_level_bit_parity(monkeypatch, rows, cols, lda):
    """Column j of cgx_matvec_nrhs is cgx_matvec(CGX_F64) on column j bit for bit, for nrhs = 1..8, and within 1e-13
    (relative, max norm) of numpy.  Below one chunk, one chunk -1 / 0 / +1, 17 chunks (no multiple of U); the odd
    pitches 7 and 127 send every column of A through the scalar tail, as does V one element off the 16-byte grid
    (v_offset = 1) and, for every other column, an odd ldv; ldv > cols throughout, ldo > rows."""
    monkeypatch.delenv("CGX_MV_NRHS_PLAN", raising=False)
    rng = np.random.default_rng(1000 * rows + cols)
    A = np.full((rows, lda), np.nan)  # the pitch padding is never read
    A[:, :cols] = rng.standard_normal((rows, cols))
    dA = cg.DeviceArray.from_host(A)
    ldo = rows + 3
    forms = [(cols + 2 + (cols & 1), 0)]  # even ldv > cols, V on the grid
    if (rows, cols) == (129, 129):
        forms += [(cols + 3, 1), (cols + 2, 0)]  # even ldv one element off the grid; odd ldv
    for ldv, off in forms:
        V = rng.standard_normal(off + MAX_NRHS * ldv)
        dV = cg.DeviceArray.from_host(V)
        Vm = V[off:].reshape(MAX_NRHS, ldv)[:, :cols]
        ref = Vm @ A[:, :cols].T
        for nrhs in range(1, MAX_NRHS + 1):
            dO = cg.DeviceArray.from_host(np.full(nrhs * ldo, np.nan))
            matVec_nrhs(dA, dV, dO, rows, cols, nrhs, lda=lda, ldv=ldv, ldo=ldo, v_offset=off)
            O = dO.to_host().reshape(nrhs, ldo)
            assert np.all(np.isnan(O[:, rows:]))  # nothing stored past a column's rows
            O = O[:, :rows]
            one = _one_by_one(dA, dV, rows, cols, lda, nrhs, ldv, off)
            assert _same_bits(O, one), (ldv, off, nrhs, np.abs(O - one).max())
            err = np.abs(O - ref[:nrhs]).max(axis=1) / np.abs(ref[:nrhs]).max(axis=1)
            assert np.all(err <= 1e-13), (ldv, off, nrhs, err)


@pytest.mark.parametrize("rows,cols,lda", [(300, 1000, 1024), (8, 2176, 2176)])
def test_kernel_level_every_plan_same_bits(monkeypatch, rows, cols, lda):
    """Every instantiated (R, U, policy) of every width gives the row sums of the default plan bit for bit
    (CGX_MV_NRHS_PLAN; a plan that is not instantiated is not taken, so the default runs)."""
    rng = np.random.default_rng(rows + cols)
    A = np.zeros((rows, lda))
    A[:, :cols] = rng.standard_normal((rows, cols))
    V = rng.standard_normal((MAX_NRHS, lda))
    dA, dV = cg.DeviceArray.from_host(A), cg.DeviceArray.from_host(V)
    for nrhs in (2, 3, 8):
        width = 2 if nrhs <= 2 else 4 if nrhs <= 4 else 8
        res = []
        for (R, U) in [(None, None)] + PLANS[width]:
            for nt in (2, 8):
                if R is None:
                    monkeypatch.delenv("CGX_MV_NRHS_PLAN", raising=False)
                else:
                    monkeypatch.setenv("CGX_MV_NRHS_PLAN", f"R={R},U={U},nt={nt}")
                dO = cg.DeviceArray(nrhs * rows)
                matVec_nrhs(dA, dV, dO, rows, cols, nrhs, lda=lda, ldv=lda)
                res.append(dO.to_host())
        assert all(_same_bits(r, res[0]) for r in res), nrhs
    monkeypatch.delenv("CGX_MV_NRHS_PLAN", raising=False)


# ---- 2. every plan of the context ----------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [3, 4, 8])
def test_context_every_plan_same_bits(nrhs):
    """n = 2100, a fixed 5-iteration run under each instantiated plan: x is the same bit for bit wherever the
    grid is the same size (the fused p.Ap adds the blocks' partials, so its last bits follow the grid; at this n
    the grid follows the rows per wave) and within rounding otherwise; a plan that is not instantiated is refused
    with -1 and leaves the plan unchanged."""
    n, seed = 2100, 8
    A, B, _, _ = system(n, seed, nrhs)
    width = 4 if nrhs <= 4 else 8
    by_grid = {}
    with cg.Solver(n, nrhs=nrhs) as s:
        assert s.nrhs == nrhs and s.info.elem_bytes == 8 and s.info.nshards == 1
        assert not s.info.flags & (cg.CGX_FUSED_ACTIVE | cg.CGX_FOLD_ACTIVE | cg.CGX_SMALL_ACTIVE)
        s.set_system(A, B)
        for (R, U) in PLANS[width]:
            for nt in (2, 8):
                s.set_matvec_plan(R, U, nt, 1)
                pl = s.matvec_plan()
                assert (pl["R"], pl["U"], pl["nt"]) == (R, U, nt)
                X, st = s.solve(np.zeros((nrhs, n)), eps=-1.0, max_iter=5)
                assert st.iterations == 5 and np.all(np.isfinite(X))
                by_grid.setdefault(pl["blocks"], []).append(X)
        for plan in [(1, 4, 8), (8, 8, 8), (4, 2, 1), (4, 2, 0), (3, 2, 8)] + ([(8, 2, 8)] if width == 8 else [(2, 4, 8)]):
            before = s.matvec_plan()
            with pytest.raises(cg.CgxError) as ei:
                s.set_matvec_plan(*plan)
            assert ei.value.code == -1 and s.matvec_plan() == before
    xs = [x for v in by_grid.values() for x in v]
    for v in by_grid.values():
        assert all(np.array_equal(x, v[0]) for x in v)
    for x in xs:
        assert all(rel(x[j], xs[0][j]) <= 1e-12 for j in range(nrhs))


# ---- 3. solve parity per column ---------------------------------------------------------------
CASES = [(1, 3, 8), (5, 3, 5), (127, 4, 3), (128, 4, 8), (129, 4, 2), (130, 5, 1), (130, 5, 4), (257, 4, 5),
         (1000, 2, 3), (2100, 8, 8), (5000, 9, 2), (8193, 4, 3)]


@pytest.mark.parametrize("n,seed,nrhs", CASES)
def test_solve_parity_per_column(n, seed, nrhs):
    A, B, XO, KO = system(n, seed, nrhs)
    with cg.Solver(n, nrhs=nrhs) as s:
        s.set_system(A, B)
        X, st = s.solve(np.zeros((nrhs, n)), eps=EPS)
        per = [s.stats_rhs(j) for j in range(nrhs)]
    assert X.shape == (nrhs, n)
    assert st.converged == 1 and st.iterations == max(KO)
    assert st.rr == max(p.rr for p in per)
    with cg.Solver(n) as one:  # the one-system context on (A, b_j): the same loop count
        one.set_system(A, B[0])
        for j in range(nrhs):
            one.set_rows(0, None, B[j])
            _, s1 = one.solve(np.zeros(n), eps=EPS)
            assert s1.iterations == KO[j], (j, s1.iterations, KO[j])
    for j in range(nrhs):
        assert per[j].converged == 1
        meets_bar(X[j], per[j].iterations, A, B[j], XO[j], KO[j])


# ---- 4. freeze ------------------------------------------------------------------------------------
def test_freeze():
    """Columns that stop at iterations 7 / 4 / 2 (and a b = 0 column, which stops at once and stays exactly
    zero): the per-column counts are the oracle's, and an early column's x is the same bits whether its
    neighbours go on iterating (large scale) or stop early too."""
    n, seed = 130, 5
    A = matrix(n, seed)
    c0, c1, c2 = (column(n, seed, j) for j in range(3))
    assert (c0[2], c1[2], c2[2]) == (7, 4, 2)
    early0 = scaled_column(n, seed, 0, 1e-9)  # column 0's b at the small scale: stops at 2
    with cg.Solver(n, nrhs=4) as s:
        s.set_system(A, np.stack([c0[0], c1[0], c2[0], np.zeros(n)]))
        X, st = s.solve(np.zeros((4, n)), eps=EPS)
        its = [s.stats_rhs(j).iterations for j in range(4)]
        conv = [s.stats_rhs(j).converged for j in range(4)]
        s.set_system(A, np.stack([early0[0], c1[0], c2[0], np.zeros(n)]))
        Y, sty = s.solve(np.zeros((4, n)), eps=EPS)
        itsy = [s.stats_rhs(j).iterations for j in range(4)]
    assert its == [7, 4, 2, 1] and conv == [1, 1, 1, 1] and st.iterations == 7 and st.converged == 1
    assert itsy == [early0[2], 4, 2, 1] and sty.iterations == 4
    assert np.array_equal(X[1], Y[1]) and np.array_equal(X[2], Y[2])
    assert not X[3].any() and not Y[3].any() and not np.signbit(X[3]).any()
    for j, c in enumerate((c0, c1, c2)):
        meets_bar(X[j], its[j], A, c[0], c[1], c[2])
    meets_bar(Y[0], itsy[0], A, early0[0], early0[1], early0[2])


# ---- 5. independence and determinism ---------------------------------------------------------------
def test_independence_and_determinism(monkeypatch):
    n, seed, nrhs = 1000, 2, 5
    A, B, _, KO = system(n, seed, nrhs)
    perm = [3, 0, 4, 2, 1]
    res = {}
    for gated in (None, "0"):
        if gated is None:
            monkeypatch.delenv("CGX_GATED", raising=False)
        else:
            monkeypatch.setenv("CGX_GATED", gated)
        with cg.Solver(n, nrhs=nrhs) as s:
            s.set_system(A, B)
            X, st = s.solve(np.zeros((nrhs, n)), eps=EPS)
            its = [s.stats_rhs(j).iterations for j in range(nrhs)]
            X2, st2 = s.solve(np.zeros((nrhs, n)), eps=EPS)
            s.set_system(A, B[perm])
            XP, _ = s.solve(np.zeros((nrhs, n)), eps=EPS)
            itp = [s.stats_rhs(j).iterations for j in range(nrhs)]
            xf, stf = s.solve(np.zeros((nrhs, n)), eps=-1.0, max_iter=9)
        res[gated] = (X, its, (st.iterations, st.converged, st.rr))
        assert its == KO
        assert np.array_equal(X, X2) and (st2.iterations, st2.converged, st2.rr) == res[gated][2]
        assert np.array_equal(XP, X[perm]) and itp == [KO[p] for p in perm]
        # a fixed count past convergence: every column has run 9 iterations, x finite
        assert stf.iterations == 9 and np.all(np.isfinite(xf))
    assert np.array_equal(res[None][0], res["0"][0]) and res[None][1:] == res["0"][1:]


def test_solve_in_pieces():
    """begin, iterate(3), iterate(100, eps) gives solve's x: every column here needs more than 3 iterations
    (7 / 4 / 7), so the three fixed ones decide nothing a tested one would not."""
    n, seed = 130, 5
    A = matrix(n, seed)
    cols = [column(n, seed, 0), column(n, seed, 1), column(n, seed, 3)]
    assert [c[2] for c in cols] == [7, 4, 7]
    B = np.stack([c[0] for c in cols])
    with cg.Solver(n, nrhs=3) as s:
        s.set_system(A, B)
        X, st = s.solve(np.zeros((3, n)), eps=EPS)
        s.set_x(np.zeros((3, n)))
        s.begin()
        d1, c1 = s.iterate(3)
        d2, c2 = s.iterate(100, eps=EPS)
        XP = s.get_x()
        its = [s.stats_rhs(j).iterations for j in range(3)]
        d3, c3 = s.iterate(5, eps=EPS)  # finished: nothing more runs
    assert (d1, c1) == (3, False) and (d1 + d2, c2) == (7, True) and (d3, c3) == (0, True)
    assert its == [7, 4, 7] and np.array_equal(XP, X)


# ---- 6. data paths -----------------------------------------------------------------------------------
def test_set_rows_in_pieces_equals_set_system():
    n, seed, nrhs = 1000, 2, 3
    A, B, _, _ = system(n, seed, nrhs)
    rng = np.random.default_rng(5)
    X0 = 1e-3 * rng.standard_normal((nrhs, n))
    with cg.Solver(n, nrhs=nrhs) as s:
        s.set_system(A, B, X0)
        Xa, sta = s.solve(None, eps=EPS)
        s.fill(0.0, 0.0)
        for lo, hi in ((0, 100), (100, 333), (333, 900), (900, n)):  # cuts at non-multiples of 128
            s.set_rows(lo, A[lo:hi], B[:, lo:hi], X0[:, lo:hi])
        Xb, stb = s.solve(None, eps=EPS)
    assert np.array_equal(Xa, Xb) and sta.iterations == stb.iterations


def test_generate_spd_fill_and_x_round_trip():
    n, seed, nrhs = 2100, 8, 3  # unscaled generator columns: 17 / 0.075 before / at the stop for every one
    A = matrix(n, seed)
    with cg.Solver(n) as one:
        one.generate_spd(seed)
        x1, s1 = one.solve(None, eps=EPS)
    with cg.Solver(n, nrhs=nrhs) as s:
        s.generate_spd(seed)
        X, st = s.solve(None, eps=EPS)
        its = [s.stats_rhs(j).iterations for j in range(nrhs)]
        rn, bn = s.residual_norms()
        with pytest.raises(cg.CgxError, match="cgx_residual_norms") as ei:
            s.residual_norm()
        assert ei.value.code == -1
        # fill and the x round trip
        s.fill(2.5, -1.25)
        assert np.array_equal(s.get_x(), np.full((nrhs, n), -1.25))
        rf, bf = s.residual_norms()
        R = np.arange(nrhs * n, dtype=np.float64).reshape(nrhs, n) * 0.5
        s.set_x(R)
        assert np.array_equal(s.get_x(), R)
    # column 0 is the one-system context's system: its loop count and the bar; column j's b is seed + j's
    assert s1.iterations == checked_oracle(A, hash_b(n, seed))[1]
    for j in range(nrhs):
        b = hash_b(n, seed + j)
        xo, Kj = checked_oracle(A, b)
        meets_bar(X[j], its[j], A, b, xo, Kj)
        assert abs(rn[j] - np.linalg.norm(b - A @ X[j])) <= 1e-12 * np.linalg.norm(b)
        assert abs(bn[j] - np.linalg.norm(b)) <= 1e-14 * np.linalg.norm(b)
    assert rel(X[0], x1) <= TOL
    want_r = np.linalg.norm(2.5 - A @ np.full(n, -1.25))
    assert np.allclose(rf, want_r, rtol=1e-13) and np.allclose(bf, 2.5 * np.sqrt(n), rtol=1e-14)


# ---- 7. offsets past 4 GiB ---------------------------------------------------------------------------
def test_byte_offsets_past_4gib():
    """n = 23296, the smallest n (lda = n, a multiple of 128) with n * lda * 8 > 2^32: the device generator, two
    systems, 3 fixed iterations.  Column 0 against oracle.cg_f64_hash (A regenerated per matVec, no n^2 memory).
    Then b_1 = 2 b_0: scaling by 2 is exact in every operation of CG, so x_1 must be 2 x_0 bit for bit -- a
    second column that indexes A or its own vectors wrongly past 2^32 bytes misses by O(1)."""
    n, seed = 23296, 7
    assert n * n * 8 > 2 ** 32 and (n - 128) * (n - 128) * 8 < 2 ** 32
    xo, so = oracle.cg_f64_hash(n, seed, max_iter=3, eps=-1.0)
    with cg.Solver(n, nrhs=2) as s:
        assert s.info.lda == n
        s.generate_spd(seed)
        X, st = s.solve(None, eps=-1.0, max_iter=3)
        s.set_rows(0, None, np.stack([hash_b_numpy(n, seed), 2.0 * hash_b_numpy(n, seed)]), np.zeros((2, n)))
        Y, _ = s.solve(None, eps=-1.0, max_iter=3)
    assert st.iterations == 3 and so.iterations == 3
    assert rel(X[0], xo) <= TOL, rel(X[0], xo)
    assert np.array_equal(Y[0], X[0]) and np.array_equal(Y[1], 2.0 * Y[0])
    assert rel(X[1], xo) > 1e-3  # column 1 is another system (seed + 1's b)


def _mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_b_numpy(n, seed):
    """spd_hash(n, seed)[1] without generating A (pinned against the oracle in test_hash_b_numpy)."""
    salt = _mix64(np.array([seed + 1], np.uint64))[0]
    return (_mix64(np.arange(n, dtype=np.uint64) ^ salt) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def test_hash_b_numpy():
    for n, seed in ((130, 5), (1000, 3)):
        assert np.array_equal(hash_b_numpy(n, seed), hash_b(n, seed))


# ---- 8. CLI --------------------------------------------------------------------------------------------
ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")


def _per_system(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("system ")]


def test_cli_nrhs(tmp_path):
    n, seed = 1000, 2
    A = matrix(n, seed)
    r = subprocess.run([cg.CLI_PATH, "--nrhs", "3", "--spd", str(n), "--seed", str(seed), "--eps", "1e-10", "--stats"],
                       capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    # The generator fixes these columns (no scale to choose): before / at the stop they stand at 51 / 0.33,
    # 54 / 0.35 and 53 / 0.34, a factor of 2.87 at the least where the chosen cases keep 3.  What has to be
    # covered is the gap between two fp64 summation orders of r.r, 1e-13 relative: a factor of 2.5 is asserted.
    want = [checked_oracle(A, hash_b(n, seed + j), margin=2.5)[1] for j in range(3)]
    assert f"iterations: {max(want)} converged: 1" in r.stdout.splitlines()[-4]  # the whole run, then the systems
    lines = _per_system(r.stdout)
    assert len(lines) == 3
    for j, ln in enumerate(lines):
        assert ln.startswith(f"system {j} iterations: {want[j]} converged: 1"), ln

    # the file form: generateSPDmatrix(512) as the MATLAB script writes it, two systems
    m, K = 512, 2
    Am, bm = oracle.spd_matlab(m, np.float64)
    Bm = np.stack([0.1 * bm, 1e-3 * bm[::-1]])  # scales at which the oracle's loop count has the margin
    for name, arr, dec in (("A.txt", Am, 4), ("b.txt", Bm, 9), ("x0.txt", np.zeros((K, m)), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    r = subprocess.run([cg.CLI_PATH, "--nrhs", str(K), "--eps", "1e-10", "--print-x", "--stats", *paths],
                       capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Computing cg of matrix size : {m * m}" in r.stdout
    X = np.array([float(v) for v in r.stdout.strip().splitlines()[-K * m:]]).reshape(K, m)
    Aw = cg.read_text(paths[0], m * m, np.float64).reshape(m, m)
    Bw = cg.read_text(paths[1], K * m, np.float64).reshape(K, m)
    lines = _per_system(r.stdout)
    assert len(lines) == K
    for j in range(K):
        xo, Kj = checked_oracle(Aw, Bw[j])
        assert lines[j].startswith(f"system {j} iterations: {Kj} converged: 1"), lines[j]
        assert rel(X[j], xo) <= TOL

    for extra in (["--fp32-ref"], ["--a-fp32"], ["--symmetric"], ["--gpus", "2"], ["--p2p"]):
        r = subprocess.run([cg.CLI_PATH, "--nrhs", "2", *extra, *paths], capture_output=True, text=True, env=ONE_GPU)
        assert r.returncode == 2 and len(r.stderr.strip().splitlines()) == 1, (extra, r.returncode, r.stderr)
    r = subprocess.run([cg.CLI_PATH, "--nrhs", "9", *paths], capture_output=True, text=True, env=ONE_GPU)
    assert r.returncode == 2 and len(r.stderr.strip().splitlines()) == 1
