"""Dense fp64 systems on which CG stops at a known, sharp iteration.

``A = Q diag(lambda) Q^T`` (symmetrised as ``(A + A.T) / 2``) with m distinct
eigenvalues ``logspace(0, 2, m)``: kappa = 100, lambda_min = 1.  Exact CG ends
after m iterations on such a matrix; in fp64 the residual falls off a cliff of
two or more orders one or two iterations later, and a stopping threshold put
in the middle of that cliff gives a loop count K >= 13 that no summation order
moves.  The entries are signed, the off-diagonal row sums are several times
the diagonal, and x0 is nonzero (the initial matVec runs).

Q is ``np.linalg.qr`` of a seeded normal matrix for n <= 2304, and a product
of three seeded Householder reflections above that (O(n^2), no QR).

Everything here is a reference in plain numpy fp64 (``history`` is
``conjgrad.m``'s order, as ``oracle.conjgrad_numpy``) -- none of it is the
code under test.  Arrays are cached and read-only.

``spread`` runs the same loop under three summation orders (BLAS; columns
permuted; 128-column partial sums) and is the measured quantity the GPU
tolerances of tests/test_gpu_long_solves.py are set from: the GPU's order is a
fourth one, so they are 100 x this spread.

Measured (printed by ``pytest -s tests/test_long_systems_cpu.py``, which also
asserts the caps T_h <= 1e-8, T_x <= 1e-10 and spread of x at F <= 1e-13):

=====  ==  ===========  ==  =========  =========  ========  ========  ================  ===========
n      m   Q            K   eps        drop at K  T_h       T_x       spread K-1..K+1   x spread, F
=====  ==  ===========  ==  =========  =========  ========  ========  ================  ===========
130    12  qr           13  7.512e-05  1382x      1.68e-13  2.57e-13  0.19 0.24 0.18    1.2e-14
1000   12  qr           13  2.162e-04  1352x      2.95e-13  6.18e-13  0.08 0.03 0.09    3.3e-14
1001   16  qr           18  5.494e-04  266x       1.18e-09  1.87e-11  0.13 0.10 0.23    3.5e-14
2304   16  qr           18  9.656e-04  405x       1.15e-09  3.14e-11  0.10 0.13 0.22    4.5e-14
4096   12  Householder  13  6.837e-04  1840x      1.51e-13  5.01e-13  1.24 0.35 0.93    4.9e-15
=====  ==  ===========  ==  =========  =========  ========  ========  ================  ===========

T_h = 100 x the largest spread of sqrt(r.r) over k <= m - 4; T_x = 100 x the
spread of x at k = m - 8; F = m + 10, where sqrt(r.r) is 2e-16 .. 1e-15 (r.r
about 1e-31: far from underflow, alpha and beta are live ratios).  The
Householder system at m = 16 (K = 18, drop 584x) measured T_h = 1.57e-08, over
the 1e-8 cap, and a spread of 1.0 around the stop, so n = 4096 uses m = 12.
The off-diagonal row sums are 9.4-14.8 (n = 130), 27-34 (1000, 1001) and 43-49
(2304) times the diagonal; 0.16-155, median 6.7, for the Householder system.
The oracle's sequential sums, a fourth order, give 0.85-1.6 times numpy's
sqrt(r.r) at K - 1 and K on the qr systems and 3.0 / 2.2 times on the
Householder one; they keep a factor of 14 or more on each side of eps
(``stop`` asserts 10).
CGX_A_F32 (``widened_a32``; the cliff does not survive rounding A to float):
at the fixed count 48 sqrt(r.r) = 9.6e-21 (n = 130) and 2.0e-15 (n = 1001) and
the orders agree on x to 1.3e-14 and 3.7e-14.
"""
import numpy as np

import oracle

QR_MAX_N = 2304

# (n, m, seed) of every system the GPU tests use
SYSTEMS = {130: (130, 12, 130), 1000: (1000, 12, 1000), 1001: (1001, 16, 1001), 2304: (2304, 16, 2304),
           4096: (4096, 12, 4096)}
A32_COUNT = 48  # CGX_A_F32: the fixed count compared (the cliff does not survive rounding A to float)
A32_SIZES = (130, 1001)

_systems, _hist, _spread, _stop = {}, {}, {}, {}


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _reflect(A, v):
    """H A H with H = I - 2 v v^T / (v.v), in O(n^2)."""
    v = v / np.linalg.norm(v)
    Av = A @ v
    vA = v @ A
    return A - 2.0 * np.outer(v, vA) - 2.0 * np.outer(Av, v) + 4.0 * (v @ Av) * np.outer(v, v)


def system(n, m, seed):
    """(A, b, x0) -- cached, read-only."""
    key = (n, m, seed)
    if key not in _systems:
        rng = np.random.default_rng(seed)
        vals = np.logspace(0, 2, m)
        lam = np.concatenate([vals, rng.choice(vals, n - m)]) if n >= m else vals[:n]
        lam = rng.permutation(lam)
        if n <= QR_MAX_N:
            Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
            A = (Q * lam) @ Q.T
        else:
            A = np.diag(lam)
            for _ in range(3):
                A = _reflect(A, rng.standard_normal(n))
        A = np.ascontiguousarray((A + A.T) / 2)
        b = rng.random(n) - 0.5
        x0 = rng.random(n) - 0.5
        _systems[key] = _ro(A, b, x0)
    return _systems[key]


def widened_a32(n):
    """(A32, A32 as float64, b, x0): SYSTEMS[n]'s A rounded to float and re-symmetrised (exactly
    symmetric in float), and the same values widened -- what CGX_A_F32 computes with."""
    key = ("a32", n)
    if key not in _systems:
        A, b, x0 = system(*SYSTEMS[n])
        A32 = A.astype(np.float32)
        A32 = np.ascontiguousarray(np.triu(A32) + np.triu(A32, 1).T)
        _systems[key] = _ro(A32, A32.astype(np.float64)) + (b, x0)
    return _systems[key]


# ---- the three summation orders --------------------------------------------------------------
class _Blas:
    def __init__(self, A):
        self.A = A

    def mv(self, p):
        return self.A @ p

    def dot(self, a, b):
        return float(a @ b)


class _Permuted(_Blas):
    def __init__(self, A):
        self.perm = np.random.default_rng(7).permutation(A.shape[0])
        self.A = np.ascontiguousarray(A[:, self.perm])

    def mv(self, p):
        return self.A @ p[self.perm]

    def dot(self, a, b):
        return float(a[self.perm] @ b[self.perm])


class _Chunked(_Blas):
    W = 128

    def mv(self, p):
        out = np.zeros(self.A.shape[0])
        for c in range(0, p.size, self.W):
            out += self.A[:, c:c + self.W] @ p[c:c + self.W]
        return out

    def dot(self, a, b):
        s = 0.0
        for c in range(0, a.size, self.W):
            s += float(a[c:c + self.W] @ b[c:c + self.W])
        return s


def _cg(op, b, x0, count):
    """conjgrad.m:1-18 for `count` iterations, no stopping test.  h[k] = sqrt(r.r) and X[k] = x after k
    iterations (k = 0: the start)."""
    x = np.array(x0, np.float64)
    r = b - op.mv(x)
    p = r.copy()
    rsold = op.dot(r, r)
    h = np.empty(count + 1)
    X = np.empty((count + 1, b.size))
    h[0], X[0] = np.sqrt(rsold), x
    for k in range(1, count + 1):
        Ap = op.mv(p)
        alpha = rsold / op.dot(p, Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        rsnew = op.dot(r, r)
        h[k], X[k] = np.sqrt(rsnew), x
        p = r + (rsnew / rsold) * p
        rsold = rsnew
    return _ro(h, X)


def _key(A, b, x0, *more):
    return (id(A), id(b), id(x0)) + more


def history(A, b, x0, count):
    """(h, X): sqrt(r.r) and x after every iteration 0..count of the plain numpy fp64 loop."""
    key = _key(A, b, x0, count)
    if key not in _hist:
        _hist[key] = (_cg(_Blas(A), b, x0, count), (A, b, x0))  # the arrays kept alive: ids stay unique
    return _hist[key][0]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def spread(A, b, x0, count):
    """(sh, sx): per iteration 0..count, the largest relative difference of sqrt(r.r) and of x among the
    three summation orders."""
    key = _key(A, b, x0, count)
    if key not in _spread:
        runs = [history(A, b, x0, count), _cg(_Permuted(A), b, x0, count), _cg(_Chunked(A), b, x0, count)]
        sh, sx = np.zeros(count + 1), np.zeros(count + 1)
        for i in range(3):
            for j in range(i + 1, 3):
                (hi, Xi), (hj, Xj) = runs[i], runs[j]
                sh = np.maximum(sh, np.abs(hi - hj) / np.minimum(hi, hj))
                d = np.linalg.norm(Xi - Xj, axis=1) / np.linalg.norm(Xj, axis=1)
                sx = np.maximum(sx, d)
        _spread[key] = (_ro(sh, sx), (A, b, x0))
    return _spread[key][0]


def cliff(A, b, x0, m):
    """K: the first iteration >= m at which sqrt(r.r) drops 100x or more."""
    h, _ = history(A, b, x0, m + 10)
    for k in range(m, m + 10):
        if h[k - 1] >= 100.0 * h[k]:
            return k
    raise AssertionError(f"no 100x drop in iterations {m}..{m + 9}: {h}")


def stop(A, b, x0, K):
    """eps = sqrt(h[K-1] * h[K]), after asserting on the references alone that it stops the loop at K
    with a factor of 10 on either side."""
    key = _key(A, b, x0, K)
    if key not in _stop:
        h, _ = history(A, b, x0, K + 1)
        eps = float(np.sqrt(h[K - 1] * h[K]))
        assert h[K] <= eps / 10, (K, h[K], eps)
        assert np.all(h[:K] >= 10 * eps), (K, h[:K].min(), eps)
        # the oracle's own loop (sequential sums: a fourth order) keeps the factor of 10 on both sides
        # of the stop too; then with the stopping test
        _, below = oracle.cg_f64(A, b, x0, max_iter=K - 1, eps=-1.0)
        _, at = oracle.cg_f64(A, b, x0, max_iter=K, eps=-1.0)
        assert below.iterations == K - 1 and np.sqrt(below.rr) >= 10 * eps, (np.sqrt(below.rr), eps)
        assert at.iterations == K and np.sqrt(at.rr) <= eps / 10, (np.sqrt(at.rr), eps)
        _, so = oracle.cg_f64(A, b, x0, eps=eps)
        assert so.iterations == K and so.converged == 1, (so.iterations, K)
        _stop[key] = eps
    return _stop[key]


def column_scales(S, nrhs):
    """(s, Ks) for an nrhs solve on long_system S: column j is (s_j b, s_j x0) with s_j a power of two (the
    reference history scales exactly), chosen from the reference so that the common S["eps"] stops the
    columns at K, K + 1 and K + 2 in a mixed order, each with a margin of 10 / sqrt(2) on both sides."""
    K, eps, h = S["K"], S["eps"], S["h"]
    Ks = [K + d for d in (2, 0, 1, 0, 2, 1, 0, 1)][:nrhs] if nrhs > 3 else [K + 1, K + 2, K][:nrhs]
    s = [float(2.0 ** np.round(np.log2(eps / np.sqrt(h[k - 1] * h[k])))) for k in Ks]
    margin = 10 / np.sqrt(2)
    for sj, k in zip(s, Ks):
        assert sj * h[k] <= eps / margin and np.all(sj * h[:k] >= margin * eps), (k, sj)
    return s, Ks


def long_system(n):
    """SYSTEMS[n] with everything the GPU tests need: a dict of A, b, x0, m, K, eps, F, the reference
    history (h, X) to F, x_direct, and the tolerances T_h / T_x (100 x the measured spread)."""
    key = ("long", n)
    if key not in _systems:
        _, m, _ = SYSTEMS[n]
        A, b, x0 = system(*SYSTEMS[n])
        K = cliff(A, b, x0, m)
        F = m + 10
        h, X = history(A, b, x0, F)
        sh, sx = spread(A, b, x0, F)
        _systems[key] = dict(n=n, m=m, A=A, b=b, x0=x0, K=K, F=F, eps=stop(A, b, x0, K), h=h, X=X, sh=sh, sx=sx,
                             x_direct=np.linalg.solve(A, b), T_h=100.0 * float(sh[:m - 4 + 1].max()),
                             T_x=100.0 * float(sx[m - 8]))
    return _systems[key]
