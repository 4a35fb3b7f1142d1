"""CPU checks of the several-RHS probe's reference and data (tests/_nrhs_probe.py): the long-double dense and band
operators against an explicit matrix, the recurrence against a direct solve, the scale by hand, the cap on every bar,
the freeze case's conditions, and that the bars tell a wrong library from a right one.  `pytest -s` prints the table
that _nrhs_probe's docstring quotes."""
import numpy as np
import pytest

import _nrhs_probe as nq

LD_EPS = float(np.finfo(nq.LD).eps)
MUTATION_CASES = [("csr", 257, 3), ("dense", 129, 3), ("csr", 513, 8), ("dense", 127, 2)]  # odd n: a tail element


@pytest.mark.parametrize("kind,n", [("csr", 80), ("dense", 80), ("dense", 1), ("csr", 3)])
def test_operators_are_the_explicit_matrix(kind, n):
    op = nq.operator(kind, n)
    A = op.dense()
    p = nq.column_data(n, 0)[1]
    assert A.shape == (n, n) and np.array_equal(A, A.T)
    off = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
    assert np.all(np.diag(A) >= 4.0) and np.all(off < 3.0)  # SPD by Gershgorin
    if kind == "dense":
        assert np.count_nonzero(A) == n * n and np.all(np.abs(A[~np.eye(n, dtype=bool)]) <= 3.0 / n)
    scale = np.abs(A) @ np.abs(p)
    for M, apply in ((A, op.apply), (np.abs(A), op.apply_abs)):
        want = M.astype(nq.LD) @ p.astype(nq.LD)
        got = apply(p.astype(nq.LD))
        assert got.dtype == nq.LD
        # n products and sums per row in long double, in whatever order: far below one fp64 ulp of |A| |p|
        assert np.all(np.abs(got - want) <= 2 * n * LD_EPS * scale)
        assert np.all(np.abs(apply(p) - M @ p) <= 2 * n * nq.ULP * scale)
    assert np.array_equal(op.apply_abs(np.abs(p)), op.apply_abs(-np.abs(p)) * -1.0)


def test_columns_do_not_depend_on_nrhs_or_kind():
    for variant in nq.VARIANTS:
        for nrhs in range(1, nq.MAX_NRHS + 1):
            cols = nq.columns("csr", 257, nrhs, variant)
            assert [c.j for c in cols] == list(range(nrhs))
            zero = [c.zero for c in cols]
            assert zero == ([True] * nrhs if variant == "zero" else [False] * (nrhs - 1) + [nrhs >= 2])
            B, X0 = nq.rhs(cols)
            assert B.shape == X0.shape == (nrhs, 257) and np.all(B != 0.0)
            for c in cols:
                assert np.array_equal(B[c.j], nq.column_data(257, c.j)[0])
                assert np.array_equal(X0[c.j], 0 * B[c.j] if c.zero else nq.column_data(257, c.j)[1])
            Bd, X0d = nq.rhs(nq.columns("dense", 257, nrhs, variant))
            assert np.array_equal(B, Bd) and np.array_equal(X0, X0d)
    b0, b1 = nq.column_data(257, 0)[0], nq.column_data(257, 1)[0]
    assert not np.array_equal(b0, b1) and np.abs(b0).max() < 0.5
    assert not nq.column(nq.Col("csr", 257, 0, False)).X[1].flags.writeable


@pytest.mark.parametrize("kind", ["csr", "dense"])
def test_recurrence_solves_a_small_system(kind):
    """n = 12: exact CG ends after at most n loops; in long double 12 loops leave a residual far below fp64 rounding
    of |b|.  nq.cg's three loops are that recurrence's, and its r.r is r . r."""
    n = 12
    op = nq.operator(kind, n)
    b, x0 = nq.column_data(n, 2)
    x = x0.astype(nq.LD)
    r = b.astype(nq.LD) - op.apply(x)
    p, rr = r.copy(), np.dot(r, r)
    X, RR = [], [rr]
    for _ in range(n):
        Ap = op.apply(p)
        alpha = rr / np.dot(p, Ap)
        x, r = x + alpha * p, r - alpha * Ap
        rr_new = np.dot(r, r)
        p, rr = r + (rr_new / rr) * p, rr_new
        X.append(x)
        RR.append(rr)
    assert np.max(np.abs(b.astype(nq.LD) - op.apply(X[-1]))) <= 1e-17 * np.max(np.abs(b))
    assert np.allclose(X[-1].astype(np.float64), np.linalg.solve(op.dense(), b), rtol=0, atol=1e-13)
    ref = nq.column(nq.Col(kind, n, 2, False))
    assert all(np.array_equal(ref.X[k], X[k - 1]) for k in nq.KS) and all(ref.RR[k] == RR[k] for k in nq.RRKS)


@pytest.mark.parametrize("kind", ["csr", "dense"])
def test_scale_is_the_sum_of_the_terms(kind):
    """S_1, R_1 and T by hand on a small case; S grows with k; x0 = 0 leaves only the steps."""
    n = 129
    col = nq.Col(kind, n, 3, False)
    ref, op = nq.column(col), nq.operator(kind, n)
    b, x0 = (a.astype(nq.LD) for a in nq.start(col))
    r0 = b - op.apply(x0)
    R0 = np.abs(b) + op.apply_abs(np.abs(x0))
    alpha0 = np.dot(r0, r0) / np.dot(r0, op.apply(r0))
    assert np.array_equal(ref.X[1], x0 + alpha0 * r0) and ref.RR[0] == np.dot(r0, r0)
    assert np.allclose(ref.S[1], (np.abs(x0) + alpha0 * R0).astype(np.float64), rtol=4 * nq.ULP, atol=0)
    assert np.isclose(ref.T[0], float(np.dot(R0, R0)), rtol=4 * nq.ULP, atol=0)
    R1 = R0 + alpha0 * op.apply_abs(R0)
    assert np.isclose(ref.T[1], float(np.dot(R1, R1)), rtol=4 * nq.ULP, atol=0)
    assert np.all(np.abs(r0) <= R0) and np.all(ref.S[1] < ref.S[2]) and np.all(ref.S[2] < ref.S[3])
    assert ref.T[0] < ref.T[1] < ref.T[2] < ref.T[3]
    for k in nq.KS:
        assert np.all(np.abs(ref.X[k]) <= ref.S[k] * (1 + 1e-15))  # x is a sum of the terms S adds up in magnitude
    for k in nq.RRKS:
        assert 0 < ref.RR[k] <= ref.T[k]
    zero = nq.column(col._replace(zero=True))
    a0 = np.dot(b, b) / np.dot(b, op.apply(b))
    assert np.array_equal(zero.X[1], a0 * b) and zero.RR[0] == np.dot(b, b)
    assert np.allclose(zero.S[1], (a0 * np.abs(b)).astype(np.float64), rtol=4 * nq.ULP, atol=0)


def test_bars_are_capped():
    print("\n" + nq.table())
    cols = [c for _, cs in nq.groups() for c in cs]
    assert len(cols) == len(set(cols)) == 16 * (len(nq.CSR_SIZES) + len(nq.DENSE_SIZES) + 1) + 3
    for c in cols:
        sp, rsp = nq.spreads(c)
        for k in nq.KS:
            assert len(sp[k]) == 3 and nq.bar(c, k) == 100.0 * max(*sp[k], nq.FLOOR)
            assert nq.FLOOR * 100 <= nq.bar(c, k) <= nq.CAP, (c, k, sp[k])
        for k in nq.RRKS:
            assert len(rsp[k]) == 3 and nq.FLOOR * 100 <= nq.rr_bar(c, k) <= nq.CAP, (c, k, rsp[k])
        assert nq.rr_loops(c.n) == tuple(k for k in nq.RRKS if k < c.n)
    assert nq.STRIDE[0] // 2 == 2048 * 1024 + 1 and nq.STRIDE[0] % 2 == 1 and nq.STRIDE[1] == 3


# ---- the probe discriminates ----------------------------------------------------------------------------------------
def misses_by(kind, n, nrhs, variant, X):
    """The largest |x - x_ld| / (bar S) over the loops, columns and elements of X (3, nrhs, n)."""
    refs = nq.references(nq.columns(kind, n, nrhs, variant))
    return max(float(np.max(nq.ratios(X[k - 1][c.j], ref.X[k], ref.S[k]))) / nq.bar(c, k)
               for k in nq.KS for c, ref in ((r.col, r) for r in refs))


@pytest.mark.parametrize("kind,n,nrhs", MUTATION_CASES)
def test_probe_discriminates(kind, n, nrhs):
    assert n % 2 == 1 and nrhs >= 2
    for variant in nq.VARIANTS:
        assert misses_by(kind, n, nrhs, variant, nq.restate_case(kind, n, nrhs, variant)) <= 0.01 + 1e-12
    least = {}
    for mutation in nq.MUTATIONS:
        # every mutation on the rough start; A x0 skipped changes nothing from x0 = 0, the others are run there too
        for variant in nq.VARIANTS:
            if variant == "zero" and mutation in ("A x0 skipped", "column pitch"):
                continue
            q = misses_by(kind, n, nrhs, variant, nq.restate_case(kind, n, nrhs, variant, mutation))
            assert q >= 1000.0, (mutation, variant, q)
            least[mutation] = min(q, least.get(mutation, np.inf))
    print(f"\n[nrhs probe] {kind} n {n} nrhs {nrhs}: the mutations miss by "
          + ", ".join(f"{m}: {q:.3g}" for m, q in least.items()) + " bars")


@pytest.mark.parametrize("kind,n", nq.FREEZE_SIZES)
def test_freeze_conditions_and_mutation(kind, n):
    """The scaled columns stop after loop 1 and the unscaled ones do not stop, with a factor of 3 on both sides, on
    the reference alone; the scaling is exact; a frozen column that takes one more x update misses by 1000 bars."""
    most, least = nq.freeze_conditions(kind, n)
    print(f"\n[nrhs probe] freeze {kind} n {n}: scaled sqrt(r1.r1) <= {most:.3g}, unscaled >= {least:.3g}, "
          f"E = {nq.FREEZE_EPS:g}")
    assert [nq.scaled_columns(p, k) for p, k in (("odd", 5), ("even", 5), ("all", 1))] == [[1, 3], [0, 2, 4], [0]]
    assert len(nq.FREEZE_PATTERNS) == 10
    op = nq.operator(kind, n)
    for col in nq.columns(kind, n, 2, "rough"):
        b, x0 = nq.start(col)
        plain, _ = nq.cg(op, b, x0, np.float64, nq.DOTS["d_at"])
        scaled, _ = nq.cg(op, b * nq.FREEZE_SCALE, x0 * nq.FREEZE_SCALE, np.float64, nq.DOTS["d_at"])
        for k in nq.KS:  # exact: CG on the scaled column is the unscaled one times 2^-40, bit for bit
            assert np.array_equal(scaled[k - 1], plain[k - 1] * nq.FREEZE_SCALE)
        ref = nq.column(col)
        frozen_right, frozen_wrong = scaled[0], scaled[1]  # x_1 kept; x_1 with one more update
        S = ref.S[1] * nq.FREEZE_SCALE
        want = ref.X[1] * nq.LD(nq.FREEZE_SCALE)
        assert float(np.max(nq.ratios(frozen_right, want, S))) <= 0.01 * nq.bar(col, 1)
        q = float(np.max(nq.ratios(frozen_wrong, want, S))) / nq.bar(col, 1)
        assert q >= 1000.0, (col, q)
        print(f"[nrhs probe] a frozen column {col.j} updated once more misses by {q:.3g} bars")
