"""Extended-precision reference and probe data for the matrix-free 5-point Poisson kernels.

numpy and ``oracle`` only -- none of it is the code under test.  Arrays are cached and read-only.

``apply_ld`` / ``cg_ld``: the operator and K fixed loops of ``conjgrad.m``'s sequential CG (no stopping test) in
``np.longdouble``.  The module refuses to load where long double has no more bits than double: a comparison
of fp64 with fp64 would say nothing about either.

``rough(m, seed)``: seeded standard-normal b and x0 -- not smooth, not symmetric under either reflection or
under transposition, both nonzero (so r0 = b - A x0 is computed from x0, and x's halo rows differ from the
neighbour's own boundary rows).

``comb(m, mloc, K)``: b = 1.0 at isolated grid points next to the edges the kernels treat specially (item
rows 7/8, slab rows mloc-1/mloc, wave columns 127/128, strip columns 511/512, the grid's own edges), any
two at Manhattan distance >= 3, x0 = 0.  After K fixed loops x lies in span{b, A b, .., A^(K-1) b}: exactly
zero outside the union of radius-(K-1) diamonds round the points (the returned mask), and after one loop
x == b / 4 bit for bit (r.r = N, p.Ap = 4 N, alpha = 0.25 exactly; N points).  A kernel that writes a stray
value, or reads a neighbour that is not one, breaks an exact zero.

``bar(m, K)``: the element-wise tolerance of tests/test_gpu_poisson_probe.py as a fraction of max|x_ld|,
by this suite's rule (tests/_long_systems.py): 100 x the measured spread between fp64 summation orders.  The
spread is the larger of two distances max|x - x_ld| / max|x_ld| on ``rough(m, m)`` after K loops: d_seq, the
oracle's sequential fp64 CG (``oracle.cg_poisson_f64(..., eps=-1, max_iter=K)``), and d_pair, a numpy fp64 CG
whose dots are numpy's pairwise sums; floored at FLOOR = 4 ulp of fp64 (8.9e-16: the m = 2 rows below measure
1.0 to 1.3 ulp and the m = 8 rows 1.2 to 8.2 ulp, so the floor lies between them and lifts only the rows that
measure less; with four points, two orders can also agree exactly, and a zero spread would give a zero bar).
The GPU's order is a third one.

Measured (printed by ``pytest -s tests/test_poisson_probe_cpu.py``, which asserts every bar <= 1e-10):

=====  ==  ========  ========  ========
m      K   d_seq     d_pair    bar
=====  ==  ========  ========  ========
2      1   2.83e-16  2.83e-16  8.88e-14
2      2   2.47e-16  2.47e-16  8.88e-14
2      3   2.87e-16  2.87e-16  8.88e-14
2      9   2.16e-16  2.16e-16  8.88e-14
8      1   2.72e-16  2.72e-16  8.88e-14
8      2   6.03e-16  6.98e-16  8.88e-14
8      3   9.17e-16  9.17e-16  9.17e-14
8      9   1.83e-15  1.75e-15  1.83e-13
9      1   4.77e-16  2.82e-16  8.88e-14
9      2   7.84e-16  4.16e-16  8.88e-14
9      3   7.12e-16  4.88e-16  8.88e-14
9      9   1.34e-15  6.81e-16  1.34e-13
130    1   1.45e-15  3.87e-16  1.45e-13
130    2   3.18e-15  9.33e-16  3.18e-13
130    3   2.49e-15  1.28e-15  2.49e-13
130    9   3.82e-15  9.14e-16  3.82e-13
514    1   1.42e-14  9.75e-16  1.42e-12
514    2   4.63e-15  9.57e-16  4.63e-13
514    3   9.91e-15  1.28e-15  9.91e-13
514    9   8.34e-15  1.02e-15  8.34e-13
1024   1   7.24e-14  7.43e-16  7.24e-12
1024   2   3.73e-14  1.23e-15  3.73e-12
1024   3   2.44e-14  1.61e-15  2.44e-12
1024   9   4.46e-14  1.38e-15  4.46e-12
1026   1   8.35e-14  1.23e-15  8.35e-12
1026   2   4.73e-14  1.07e-15  4.73e-12
1026   3   4.55e-14  1.47e-15  4.55e-12
1026   9   1.11e-13  1.05e-15  1.11e-11
=====  ==  ========  ========  ========
"""
import functools

import numpy as np

import oracle

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, (
    f"np.longdouble has eps = {np.finfo(LD).eps:.3g} on this machine: no extended precision, the Poisson probe "
    "reference would compare fp64 with fp64")

ULP = float(np.finfo(np.float64).eps)
FLOOR = 4 * ULP
KS = (1, 2, 3, 9)  # every residue of the x deferral (flush with one and two p slabs), then three full catch-ups
SIZES = (2, 8, 9, 130, 514, 1024, 1026)  # every grid the GPU tests run
CAP = 1e-10  # this suite's TOL: every bar stays under it
# b = 1, x0 = 0, eps = 1e-10: the largest even m <= 130 at which the oracle alone stands a factor of 3 on both sides of
# eps at its stop (_pcg_ref.checked_reference's rule).  At m = 130 (test_poisson_matches_oracle's case, 294 loops)
# sqrt(r.r) / eps is 1.05 one loop before the stop and 0.83 at it: the residual falls by about 0.8 per loop on every
# even grid from 16 to 130, so a summation order may move the count there.  m = 14: 27 loops, 5.2 before, 0.072 at.
CONVERGE_M, CONVERGE_EPS, MARGIN = 14, 1e-10, 3.0

ROWS = lambda m, mloc: (0, 3, 4, 7, 8, mloc - 1, mloc, m - 1)  # noqa: E731
COLS = lambda m: (0, 1, 2, 126, 127, 128, 255, 256, 511, 512, m - 2, m - 1)  # noqa: E731


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _apply(m, p):
    """4 c - up - dn - left - right in p's own type."""
    P = p.reshape(m, m)
    out = 4 * P
    out[1:] -= P[:-1]
    out[:-1] -= P[1:]
    out[:, 1:] -= P[:, :-1]
    out[:, :-1] -= P[:, 1:]
    return out.reshape(-1)


def apply_ld(m, p):
    """A p in long double."""
    return _apply(m, np.asarray(p, LD))


def _cg(m, b, x0, K, dtype, dot):
    """conjgrad.m:1-18 for K loops with no stopping test, in `dtype` with the given dot; x after every loop 0..K."""
    b = np.asarray(b, dtype)
    x = np.array(x0, dtype)
    r = b - _apply(m, x)
    p = r.copy()
    rsold = dot(r, r)
    X = [x]
    for _ in range(K):
        Ap = _apply(m, p)
        alpha = rsold / dot(p, Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        rsnew = dot(r, r)
        X.append(x)
        p = r + (rsnew / rsold) * p
        rsold = rsnew
    return X


def _dot_seq(a, b):
    return np.dot(a, b)  # long double: numpy's plain loop, one element after the other


def _dot_pair(a, b):
    return np.sum(a * b)  # numpy's pairwise summation


def cg_ld(m, b, x0, K):
    """x after K fixed loops of sequential CG in long double."""
    return _cg(m, b, x0, K, LD, _dot_seq)[K]


@functools.lru_cache(maxsize=None)
def rough(m, seed):
    """(b, x0): seeded standard-normal, read-only."""
    rng = np.random.default_rng(seed)
    return _ro(rng.standard_normal(m * m), rng.standard_normal(m * m))


@functools.lru_cache(maxsize=None)
def comb_points(m, mloc):
    """The thinned probe points as (row, col) pairs.  Greedy over the candidates row by row, keeping a point
    when it is at Manhattan distance >= 3 from every point kept so far: a candidate that is dropped is within
    distance 2 of a kept one, i.e. inside the K = 3 mask.  The columns are tried ascending in every other
    candidate row and descending in the rest, so both sides of a wave edge (126 | 128) and of a strip edge
    (511 | 512) are taken in some row, and both rows of a slab edge keep points."""
    rows = sorted({r for r in ROWS(m, mloc) if 0 <= r < m})
    cols = sorted({c for c in COLS(m) if 0 <= c < m})
    kept = []
    for ri, r in enumerate(rows):
        for c in (cols if ri % 2 == 0 else cols[::-1]):
            if all(abs(r - r2) + abs(c - c2) >= 3 for r2, c2 in kept):
                kept.append((r, c))
    return tuple(kept)


@functools.lru_cache(maxsize=None)
def comb(m, mloc, K=3):
    """(b, x0, mask): b = 1.0 at comb_points, x0 = 0, and the boolean mask (flat, m*m) of the union of the
    radius-(K-1) diamonds round the points."""
    pts = comb_points(m, mloc)
    b = np.zeros((m, m))
    mask = np.zeros((m, m), bool)
    for r, c in pts:
        b[r, c] = 1.0
        for dr in range(-(K - 1), K):
            w = K - 1 - abs(dr)
            if 0 <= r + dr < m:
                mask[r + dr, max(0, c - w):c + w + 1] = True
    return _ro(b.reshape(-1), np.zeros(m * m), mask.reshape(-1))


@functools.lru_cache(maxsize=None)
def _ld_runs(m, kind, mloc=0):
    """x_ld after each K of KS (long double), for rough(m, m) or comb(m, mloc)."""
    b, x0 = rough(m, m) if kind == "rough" else comb(m, mloc)[:2]
    X = _cg(m, b, x0, max(KS), LD, _dot_seq)
    return {K: _ro(X[K])[0] for K in KS}


@functools.lru_cache(maxsize=None)
def reference(m, kind, K, mloc=0):
    """(x_ld, ||b - A x_ld||, ||b||) in long double after K fixed loops on rough(m, m) / comb(m, mloc)."""
    b = (rough(m, m) if kind == "rough" else comb(m, mloc))[0]
    x = _ld_runs(m, kind, mloc)[K]
    bl = np.asarray(b, LD)
    res = bl - apply_ld(m, x)
    return x, np.sqrt(np.dot(res, res)), np.sqrt(np.dot(bl, bl))


def dist(x, x_ld):
    """max|x - x_ld| / max|x_ld|, formed in long double."""
    return float(np.max(np.abs(np.asarray(x, LD) - x_ld)) / np.max(np.abs(x_ld)))


@functools.lru_cache(maxsize=None)
def spreads(m):
    """{K: (d_seq, d_pair)} on rough(m, m)."""
    b, x0 = rough(m, m)
    ld = _ld_runs(m, "rough")
    pair = _cg(m, b, x0, max(KS), np.float64, _dot_pair)
    out = {}
    for K in KS:
        xs, st = oracle.cg_poisson_f64(m, b, x0, max_iter=K, eps=-1.0)
        assert st.iterations == K
        out[K] = (dist(xs, ld[K]), dist(pair[K], ld[K]))
    return out


def bar(m, K):
    """The element-wise tolerance after K fixed loops on an m x m grid, as a fraction of max|x_ld|."""
    return 100.0 * max(*spreads(m)[K], FLOOR)


def table():
    """The docstring's table, measured now."""
    rule = "=====  ==  ========  ========  ========"
    lines = [rule, "m      K   d_seq     d_pair    bar", rule]
    for m in SIZES:
        for K in KS:
            ds, dp = spreads(m)[K]
            lines.append(f"{m:<5d}  {K:<2d}  {ds:.2e}  {dp:.2e}  {bar(m, K):.2e}")
    return "\n".join(lines + [rule])


@functools.lru_cache(maxsize=None)
def stop_margin(m, eps=CONVERGE_EPS):
    """(x, K, sqrt(r.r) / eps one loop before the stop, at the stop) of the oracle on b = 1, x0 = 0."""
    n = m * m
    b, x0 = np.ones(n), np.zeros(n)
    x, so = oracle.cg_poisson_f64(m, b, x0, eps=eps)
    K = so.iterations
    _, before = oracle.cg_poisson_f64(m, b, x0, eps=-1.0, max_iter=K - 1)
    _, at = oracle.cg_poisson_f64(m, b, x0, eps=-1.0, max_iter=K)
    return _ro(x)[0], K, float(np.sqrt(before.rr) / eps), float(np.sqrt(at.rr) / eps)


def keeps_margin(m):
    _, _, before, at = stop_margin(m)
    return before >= MARGIN and at <= 1.0 / MARGIN
