"""The long-solve systems of tests/_long_systems.py, checked on the references alone (no GPU): every
system the GPU tests use has a sharp stop at K >= 13 on which the numpy loop and the oracle agree, and the
spread among three summation orders leaves the tolerances of tests/test_gpu_long_solves.py their stated
room.  Run with -s to see the measured spreads (recorded in _long_systems.py's docstring)."""
import numpy as np
import pytest

import _long_systems as ls
import oracle


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle.lib()


@pytest.mark.parametrize("n", sorted(ls.SYSTEMS))
def test_system_shape(n):
    _, m, seed = ls.SYSTEMS[n]
    A, b, x0 = ls.system(n, m, seed)
    assert ls.system(n, m, seed)[0] is A and not A.flags.writeable and not b.flags.writeable
    assert np.array_equal(A, A.T) and x0.any() and np.all(np.abs(b) <= 0.5) and np.all(np.abs(x0) <= 0.5)
    lam = np.linalg.eigvalsh(A)
    want = np.logspace(0, 2, m)
    near = np.abs(lam[:, None] - want[None, :]).min(axis=1)
    assert near.max() <= 1e-10 and abs(lam[0] - 1.0) <= 1e-12  # m clusters; lambda_min = 1
    assert np.unique(np.abs(lam[:, None] - want[None, :]).argmin(axis=1)).size == m  # each value used
    d = np.abs(np.diag(A))
    off = np.abs(A).sum(axis=1) - d
    assert (A < 0).any() and np.median(off / d) >= 3.0  # signed, off-diagonal heavy
    print(f"\nn={n} m={m}: off-diagonal row sum / diagonal {np.min(off / d):.2f} .. {np.max(off / d):.1f} "
          f"(median {np.median(off / d):.1f})")


@pytest.mark.parametrize("n", sorted(ls.SYSTEMS))
def test_stop_and_spread(n):
    S = ls.long_system(n)
    m, K, F, h, sh, sx = S["m"], S["K"], S["F"], S["h"], S["sh"], S["sx"]
    assert m - 4 >= 8 and K >= 13 and K >= m
    eps = ls.stop(S["A"], S["b"], S["x0"], K)  # asserts the margins and the oracle's loop count
    assert eps == S["eps"] and h[K - 1] >= 100 * h[K]
    print(f"\nn={n} m={m} K={K} eps={eps:.3e} drop at K {h[K - 1] / h[K]:.0f}x  "
          f"T_h={S['T_h']:.2e} T_x={S['T_x']:.2e}  spread at K-1..K+1 "
          f"{sh[K - 1]:.2f} {sh[K]:.2f} {sh[K + 1]:.2f}  spread of x at F={F}: {sx[F]:.1e}  h[F]={h[F]:.1e}")
    # the orders move sqrt(r.r) around the stop by less than 2.5x: the factor of 10 keeps 4x in hand
    assert sh[K - 1:K + 2].max() <= 1.5
    # fixed count F: r.r has not underflowed (alpha, beta are live ratios); the orders agree on x
    assert h[F] ** 2 > 1e-200 and h[F] > 0 and sx[F] <= 1e-13
    # history: T_h over k <= m - 4, T_x at m - 8
    assert S["T_h"] == 100 * sh[:m - 3].max() and S["T_x"] == 100 * sx[m - 8]
    assert S["T_h"] <= 1e-8 and S["T_x"] <= 1e-10
    # the direct solve is the solution the stop is measured against: lambda_min = 1
    assert np.linalg.norm(S["b"] - S["A"] @ S["x_direct"]) <= 1e-10
    assert np.linalg.norm(S["X"][K] - S["x_direct"]) <= eps * 1.01


@pytest.mark.parametrize("n", ls.A32_SIZES)
def test_a32_fixed_count(n):
    """CGX_A_F32's matrix: rounding A to float destroys the clustered spectrum (no cliff), so a fixed count
    of 48 live iterations is compared; the orders agree there to 1e-13."""
    A32, Aw, b, x0 = ls.widened_a32(n)
    assert A32.dtype == np.float32 and np.array_equal(A32, A32.T) and np.array_equal(Aw, A32.astype(np.float64))
    h, _ = ls.history(Aw, b, x0, ls.A32_COUNT)
    _, sx = ls.spread(Aw, b, x0, ls.A32_COUNT)
    print(f"\nn={n}: sqrt(r.r) at {ls.A32_COUNT} = {h[-1]:.1e}, spread of x {sx[-1]:.1e}")
    assert h[-1] ** 2 > 1e-200 and sx[-1] <= 1e-13


@pytest.mark.parametrize("n,nrhs", [(130, 8), (130, 3), (1000, 8), (1000, 3)])
def test_column_scales(n, nrhs):
    S = ls.long_system(n)
    s, Ks = ls.column_scales(S, nrhs)
    assert len(set(Ks)) >= 3 and min(Ks) >= 13 and len(Ks) == nrhs
    assert all(np.frexp(v)[0] == 0.5 for v in s)  # powers of two: the reference history scales exactly
    h = ls.history(S["A"], S["b"], S["x0"], max(Ks) + 1)[0]
    m = 10 / np.sqrt(2)
    for sj, Kj in zip(s, Ks):
        assert sj * h[Kj] <= S["eps"] / m and np.all(sj * h[:Kj] >= m * S["eps"])
        xo, so = oracle.cg_f64(S["A"], sj * S["b"], sj * S["x0"], eps=S["eps"])
        assert so.iterations == Kj
