"""CPU checks of the Poisson probe's reference and data (tests/_poisson_probe.py): the long-double operator
against the explicit matrix, the comb's exact properties on the fp64 oracle, and the cap on every bar.
`pytest -s` prints the table that _poisson_probe's docstring quotes."""
import numpy as np
import pytest

import _poisson_probe as pp
import oracle


@pytest.mark.parametrize("m", [5, 8])
def test_apply_ld_is_the_explicit_matrix(m):
    p = pp.rough(m, 11)[0]
    want = oracle.poisson_dense(m).astype(pp.LD) @ p.astype(pp.LD)
    got = pp.apply_ld(m, p)
    assert got.dtype == pp.LD
    # five products and four sums per point in long double: a few of its ulps of the largest term
    assert np.max(np.abs(got - want)) <= 8 * float(np.finfo(pp.LD).eps) * 4 * np.max(np.abs(p))
    assert np.max(np.abs(got.astype(np.float64) - oracle.poisson_apply(m, p))) <= 8 * pp.ULP * 4 * np.max(np.abs(p))


def test_cg_ld_solves_a_small_grid():
    """Exact CG ends after at most m*m loops; in long double, 16 loops on m = 4 leave a residual far below fp64."""
    m = 4
    b, x0 = pp.rough(m, 3)
    x = pp.cg_ld(m, b, x0, 16)
    assert np.max(np.abs(b.astype(pp.LD) - pp.apply_ld(m, x))) <= 1e-17 * np.max(np.abs(b))
    assert np.allclose(x.astype(np.float64), np.linalg.solve(oracle.poisson_dense(m), b), rtol=0, atol=1e-13)


def test_rough_is_rough():
    b, x0 = pp.rough(130, 130)
    B = b.reshape(130, 130)
    assert not b.flags.writeable and not x0.flags.writeable and np.all(b != 0) and np.all(x0 != 0)
    for other in (B[::-1], B[:, ::-1], B.T):
        assert np.max(np.abs(B - other)) > 1.0
    assert pp.rough(130, 130)[0] is b


@pytest.mark.parametrize("m,mloc", [(2, 2), (2, 1), (8, 1), (130, 65), (514, 257), (514, 514), (1024, 512),
                                    (1026, 1026)])
def test_comb_properties(m, mloc):
    pts = pp.comb_points(m, mloc)
    for i, (r, c) in enumerate(pts):
        assert all(abs(r - r2) + abs(c - c2) >= 3 for r2, c2 in pts[:i])
    b, x0, mask3 = pp.comb(m, mloc, 3)
    assert b.sum() == len(pts) and not x0.any()
    # every candidate point that was thinned away lies inside the K = 3 mask
    M3 = mask3.reshape(m, m)
    for r in pp.ROWS(m, mloc):
        for c in pp.COLS(m):
            if 0 <= r < m and 0 <= c < m:
                assert M3[r, c], (r, c)
    if m >= 514:  # both sides of a wave edge, of a strip edge and of the slab edge carry points of their own
        B = b.reshape(m, m)
        for side in (B[:, 126:128], B[:, 128], B[:, 511], B[:, 512:514]):
            assert side.any()
        for r in ({mloc - 1, mloc} if mloc < m else {m - 1}):
            assert B[r].any(), r
    for K in (1, 2, 3):
        _, _, mask = pp.comb(m, mloc, K)
        x, st = oracle.cg_poisson_f64(m, b, x0, max_iter=K, eps=-1.0)
        assert st.iterations == K
        assert not x[~mask].any(), (K, np.flatnonzero(x * ~mask)[:5])
        assert np.all(x[mask] != 0.0), K
        if K == 1:
            assert np.array_equal(x, b / 4)
            assert np.array_equal(mask, b != 0)
        xl = pp.reference(m, "comb", K, mloc)[0]
        assert not xl[~mask].any() and np.all(xl[mask] != 0)


def test_bars_are_capped():
    for m in pp.SIZES:
        for K in pp.KS:
            ds, dp = pp.spreads(m)[K]
            assert pp.bar(m, K) == 100.0 * max(ds, dp, pp.FLOOR)
            assert pp.FLOOR * 100 <= pp.bar(m, K) <= pp.CAP, (m, K, ds, dp)
    # the floor is taken from the m = 2 and m = 8 rows: a few ulps, between what the two grids measure
    worst = {m: max(max(v) for v in pp.spreads(m).values()) for m in (2, 8)}
    assert worst[2] <= pp.FLOOR <= worst[8] <= 16 * pp.ULP, worst
    print("\n" + pp.table())


def test_converging_grid_is_the_nearest_that_keeps_the_margin():
    """test_plans_converge_alike asserts a loop count: only where the oracle alone keeps a factor of 3 on both
    sides of eps at its stop.  m = 130 does not; CONVERGE_M is the nearest even m below it that does."""
    assert not pp.keeps_margin(130)
    kept = [m for m in range(130, 0, -2) if pp.keeps_margin(m)]
    assert kept[0] == pp.CONVERGE_M, kept
    _, K, before, at = pp.stop_margin(pp.CONVERGE_M)
    print(f"\nm = {pp.CONVERGE_M}: {K} loops, sqrt(r.r) / eps {before:.3g} before the stop, {at:.3g} at it; "
          f"m = 130: {pp.stop_margin(130)[1:]}")
