"""Extended-precision reference and probe data for the several-right-hand-side CG iteration (cgx_create_nrhs,
cgx_create_csr_nrhs: the K-column vector kernels of csrc/cgx_matvec_nrhs.hip and the start of csrc/cgx_nrhs.hip).

numpy only -- none of it is the code under test.  Cached arrays are read-only.  The module refuses to load where long
double has no more bits than double (tests/_pcg_probe.py's rule, whose constants and banded system it reuses).

The probe: begin, then three fixed loops (eps = -1) of plain CG on every column, x read after each loop and the
recurrence's r.r (stats_rhs(j).rr) after begin and after each loop.  x_1 = x_0 + alpha_0 r_0 shows the start kernel's
r = b - A x0 row by row; x_2 and x_3 show the r update and the x / p update, with the beta from the ring slots.

Systems.  ``operator("csr", n)``: ``_pcg_probe.system(n)``, banded (diagonal 4 + u, bands at 1, 2 and 37), SPD by
strict diagonal dominance.  ``operator("dense", n)``: symmetric, seeded by [n, 5], diagonal in [4, 5), every
off-diagonal entry nonzero in [-0.5, 0.5) * 6 / n: a row's off-diagonal magnitudes sum to less than 3, so A is SPD by
Gershgorin.  Column j: b_j and x0_j seeded by [n, j, 9] in [-0.5, 0.5), all nonzero, the same for both kinds and for
every nrhs, so a column's reference is cached per ``Col(kind, n, j, zero)`` and shared by every nrhs.

Variants of the start (``columns(kind, n, nrhs, variant)``): "zero", every column from x0 = 0 (the start that skips
A x0); "rough", every column rough except that for nrhs >= 2 the last column's x0 is exactly 0 -- one zero column
must not trigger the skip.

``column(col)``: x_ld after each of the loops 1..3 and r_k . r_k for k = 0..3 in np.longdouble (plain CG stated
sequentially, alpha and beta by the library's rule that 0 / 0 is 0; the sizes n <= 3 run past exact convergence, which
the scale absorbs), the per-element scale S_k and the scale of r.r, T_k:
    R_0 = |b| + |A| |x0|,   P_0 = R_0,   S_0 = |x0|,
    S_(m+1) = S_m + |alpha_m| P_m,   R_(m+1) = R_m + |alpha_m| |A| P_m,   P_(m+1) = R_(m+1) + |beta_(m+1)| P_m,
    T_k = sum_i R_k[i]^2,
the magnitude of every term that was added into x_i (into r_i for R), carried through A as well; |A| is the operator
with absolute entries.  S_k > 0 is asserted everywhere.

``bar(col, k)``, ``rr_bar(col, k)``: the tolerances of tests/test_gpu_nrhs_probe.py, |x[i] - x_ld[i]| <= bar S_k[i]
for every i and |rr - rr_ld| <= rr_bar T_k: this suite's rule, 100 x the measured spread between fp64 summation
orders, floored at 4 ulp.  The spread is the largest |x_f64 - x_ld| / S (|rr_f64 - rr_ld| / T) over three fp64
restatements of the recurrence that differ only in their dots: numpy's ``@``, ``@`` on the reversed vectors, and the
strictly sequential ``cumsum``.  The kernels' order is a fourth one.  r.r is compared only at loops k < n: past exact
convergence it is rounding noise.

Measured (printed by ``pytest -s tests/test_nrhs_probe_cpu.py``, which asserts every bar <= 1e-10).  A row is the
worst of its (kind, n) over the columns j = 0..7, both starts and the loops (x: k = 1..3; r.r: k = 0..min(3, n - 1));
the last row has the three columns of the capped-grid case only:

=================  ========  ========  ========  ========  ========
cases              d_at      d_rev     d_seq     bar       rr bar
=================  ========  ========  ========  ========  ========
csr n=1            1.74e-16  1.74e-16  1.74e-16  8.88e-14  8.88e-14
csr n=2            3.00e-16  1.70e-16  1.70e-16  8.88e-14  8.88e-14
csr n=3            3.16e-16  3.87e-16  3.87e-16  8.88e-14  8.88e-14
csr n=255          8.24e-16  9.30e-16  1.53e-15  1.53e-13  1.02e-13
csr n=256          3.43e-16  1.40e-15  1.75e-15  1.75e-13  8.89e-14
csr n=257          5.04e-16  8.86e-16  1.13e-15  1.13e-13  8.88e-14
csr n=511          7.58e-16  2.12e-15  1.56e-15  2.12e-13  1.66e-13
csr n=512          3.90e-16  3.58e-15  2.15e-15  3.58e-13  1.42e-13
csr n=513          3.17e-16  1.87e-15  2.02e-15  2.02e-13  1.50e-13
csr n=2047         8.65e-16  3.60e-15  4.09e-15  4.09e-13  2.22e-13
csr n=2048         4.45e-16  6.33e-15  6.00e-15  6.33e-13  3.36e-13
csr n=2049         4.44e-16  3.70e-15  6.06e-15  6.06e-13  2.34e-13
csr n=4097         4.69e-16  8.02e-15  4.59e-15  8.02e-13  3.75e-13
dense n=1          2.06e-16  2.06e-16  2.06e-16  8.88e-14  8.88e-14
dense n=2          2.55e-16  2.55e-16  2.55e-16  8.88e-14  8.88e-14
dense n=3          2.17e-16  3.35e-16  2.15e-16  8.88e-14  8.88e-14
dense n=127        6.83e-16  1.43e-15  1.30e-15  1.43e-13  8.88e-14
dense n=128        3.60e-16  1.08e-15  9.95e-16  1.08e-13  8.88e-14
dense n=129        4.42e-16  6.07e-16  6.80e-16  8.88e-14  8.88e-14
dense n=130        3.60e-16  9.82e-16  6.43e-16  9.82e-14  8.88e-14
dense n=257        5.75e-16  1.27e-15  7.55e-16  1.27e-13  8.88e-14
dense n=513        8.84e-16  1.57e-15  1.94e-15  1.94e-13  1.50e-13
dense n=1025       1.24e-15  2.85e-15  2.35e-15  2.85e-13  1.44e-13
csr n=4194307      1.09e-15  7.19e-14  9.14e-14  9.14e-12  8.24e-12
=================  ========  ========  ========  ========  ========

The mutations of tests/test_nrhs_probe_cpu.py (a neighbour's alpha, the odd tail left out of the p update, a wrong
column pitch, A x0 skipped, beta one ring slot late, a pad column's b written back) each move some element of some
x_k by at least 6.9e10 bars; a frozen column that takes one more x update misses its x_1 by at least 1.4e12 bars.
"""
import collections
import concurrent.futures

import numpy as np

import _pcg_probe as pp

LD, ULP, FLOOR, CAP, KS, SMALL = pp.LD, pp.ULP, pp.FLOOR, pp.CAP, pp.KS, pp.SMALL
RRKS = (0,) + KS
MAX_NRHS = 8
VARIANTS = ("rough", "zero")

CSR_SIZES = (1, 2, 3, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097)  # the pair loop's and the reduction's edges
DENSE_SIZES = (1, 2, 3, 127, 128, 129, 130, 257, 513)  # lda padded and not, odd and even
PLAN_DENSE = (1025, (2, 3, 8))  # (n, the nrhs): 9 chunks of 128, a multiple of no U
PLAN_CSR = (2049, (3, 8))
STRIDE = (2 * 2048 * 1024 + 3, 3)  # (n, nrhs): pairs past 2048 blocks * 1024, an odd tail, one pad column
FREEZE_SCALE = 2.0 ** -40
FREEZE_EPS = 1e-6
FREEZE_SIZES = (("csr", 257), ("dense", 129))

# kind: "csr" or "dense"; j: the column's seed; zero: x0 = 0
Col = collections.namedtuple("Col", "kind n j zero")


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


class _Banded:
    """_pcg_probe.system(n) and the same bands with absolute entries."""
    kind = "csr"

    def __init__(self, n):
        self.n, self.sys = n, pp.system(n)
        self._abs = object.__new__(pp.System)  # the same apply on |diag| and |bands|
        self._abs.n, self._abs._typed = n, {}
        self._abs.diag = np.abs(self.sys.diag)
        self._abs.off = {d: np.abs(c) for d, c in self.sys.off.items()}
        for dtype in (LD, np.float64):  # the typed bands, before threads read them (|A| is applied in fp64 only)
            self.sys.apply(np.zeros(n, dtype))
        self._abs.apply(np.zeros(n))

    def apply(self, p):
        return self.sys.apply(p)

    def apply_abs(self, p):
        return self._abs.apply(p)

    def csr(self):
        return self.sys.csr()

    def dense(self):
        return self.sys.dense()


class _Dense:
    """Symmetric, diagonal in [4, 5), every off-diagonal entry nonzero in [-0.5, 0.5) * 6 / n."""
    kind = "dense"

    def __init__(self, n):
        rng = np.random.default_rng([n, 5])
        U = np.triu((rng.random((n, n)) - 0.5) * (6.0 / n), 1)
        A = U + U.T
        A[np.arange(n), np.arange(n)] = 4.0 + rng.random(n)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(A, A.T) and np.all(A[off] != 0.0) and np.all(np.abs(A[off]) <= 3.0 / n)
        assert np.all((np.abs(A) * off).sum(axis=1) < 3.0) and np.diag(A).min() >= 4.0 and np.diag(A).max() < 5.0
        self.n, self.A = n, _ro(A)[0]
        self._typed = {np.dtype(np.float64): self.A, np.dtype(LD): _ro(A.astype(LD))[0]}
        self._abs = _ro(np.abs(A))[0]

    def apply(self, p):
        return self._typed[p.dtype] @ p

    def apply_abs(self, p):
        return self._abs @ p

    def dense(self):
        return self.A


_OPS, _LARGE_OP = {}, {}


def operator(kind, n):
    """The operator of (kind, n); of those above SMALL rows only the last one is kept."""
    kept = _OPS if n <= SMALL else _LARGE_OP
    if (kind, n) not in kept:
        if n > SMALL:
            _LARGE_OP.clear()
        kept[kind, n] = (_Banded if kind == "csr" else _Dense)(n)
    return kept[kind, n]


_DATA = {}


def column_data(n, j):
    """(b_j, x0_j) of n rows: the same for both kinds and for every nrhs."""
    if (n, j) in _DATA:
        return _DATA[n, j]
    rng = np.random.default_rng([n, j, 9])
    b, x0 = rng.random(n) - 0.5, rng.random(n) - 0.5
    assert np.all(b != 0.0) and np.all(x0 != 0.0)
    if n <= SMALL:
        _DATA[n, j] = _ro(b, x0)
    return b, x0


def start(col):
    """(b, x0) of a column."""
    b, x0 = column_data(col.n, col.j)
    return b, (np.zeros(col.n) if col.zero else x0)


def columns(kind, n, nrhs, variant):
    """The nrhs columns of a case: "zero", all from x0 = 0; "rough", all rough but the last of nrhs >= 2."""
    assert variant in VARIANTS and 1 <= nrhs <= MAX_NRHS
    return [Col(kind, n, j, variant == "zero" or (nrhs >= 2 and j == nrhs - 1)) for j in range(nrhs)]


def rhs(cols):
    """(B, X0), each (nrhs, n), of a case's columns."""
    pairs = [start(c) for c in cols]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


_ratio = pp._ratio  # num / den, 0 where the system is solved exactly (0 / 0): the kernels' cg_ratio


def cg(op, b, x0, dtype, dot, scales=False):
    """Plain CG in `dtype` with the given dot, no stopping test: (x after each of the loops 1..3, r_k . r_k for
    k = 0..3); with `scales` also (S_1..S_3, T_0..T_3)."""
    b = b.astype(dtype)
    x = x0.astype(dtype)
    r = b - op.apply(x)
    p = r.copy()
    rr = dot(r, r)
    X, RR, S, T = [], [rr], [], []
    if scales:  # the scales in fp64: they are magnitudes, a rounding of theirs moves no bar
        R = np.abs(b).astype(np.float64) + op.apply_abs(np.abs(x).astype(np.float64))
        P, s = R, np.abs(x).astype(np.float64)
        T.append(float(R @ R))
    for _ in KS:
        Ap = op.apply(p)
        alpha = _ratio(rr, dot(p, Ap))
        x = x + alpha * p
        r = r - alpha * Ap
        rr_new = dot(r, r)
        beta = _ratio(rr_new, rr)
        X.append(x)
        RR.append(rr_new)
        if scales:
            s = s + float(abs(alpha)) * P
            R = R + float(abs(alpha)) * op.apply_abs(P)
            P = R + float(abs(beta)) * P
            S.append(s)
            T.append(float(R @ R))
        p = r + beta * p
        rr = rr_new
    return (X, RR, S, T) if scales else (X, RR)


DOTS = pp.DOTS  # d_at, d_rev, d_seq


def ratios(x, x_ld, S):
    """|x - x_ld| / S per element; the difference is formed in long double."""
    return np.abs(np.asarray(x, LD) - x_ld).astype(np.float64) / S


def rr_loops(n):
    """The loops at which r.r is compared: k < n."""
    return tuple(k for k in RRKS if k < n)


# X, S: {k: array} for k = 1..3; RR (long double), T (fp64): {k: scalar} for k = 0..3;
# spread, rr_spread: {k: (d_at, d_rev, d_seq)}
Ref = collections.namedtuple("Ref", "col X S RR T spread rr_spread")
_REFS, _SPREADS = {}, {}


def _reference(col, pool):
    """The futures of a column's four runs."""
    op = operator(col.kind, col.n)
    b, x0 = start(col)
    return (pool.submit(cg, op, b, x0, LD, np.dot, True),
            [pool.submit(cg, op, b, x0, np.float64, dot) for dot in DOTS.values()])


def _finish(col, ld, f64):
    X, RR, S, T = ld.result()
    assert all(np.all(s > 0) for s in S) and all(t > 0 for t in T)
    spread, rr_spread = {k: [] for k in KS}, {k: [] for k in RRKS}
    for fut in f64:
        Xf, RRf = fut.result()
        for k in KS:
            spread[k].append(float(np.max(ratios(Xf[k - 1], X[k - 1], S[k - 1]))))
        for k in RRKS:
            rr_spread[k].append(float(abs(LD(RRf[k]) - RR[k]) / T[k]) if k < col.n else 0.0)
    _SPREADS[col] = ({k: tuple(v) for k, v in spread.items()}, {k: tuple(v) for k, v in rr_spread.items()})
    ref = Ref(col, {k: _ro(X[k - 1])[0] for k in KS}, {k: _ro(S[k - 1])[0] for k in KS},
              {k: RR[k] for k in RRKS}, {k: float(T[k]) for k in RRKS}, *_SPREADS[col])
    if col.n <= SMALL:
        _REFS[col] = ref
    return ref


def references(cols):
    """The references of several columns, the runs of those not cached side by side (they are independent)."""
    todo = [c for c in dict.fromkeys(cols) if c not in _REFS]
    if todo:
        for c in todo:
            operator(c.kind, c.n)  # built once, before the threads
        with concurrent.futures.ThreadPoolExecutor(min(16, 4 * len(todo))) as pool:
            futs = [(c, *_reference(c, pool)) for c in todo]
            made = {c: _finish(c, ld, f64) for c, ld, f64 in futs}
    return [_REFS[c] if c in _REFS else made[c] for c in cols]


def column(col):
    return references([col])[0]


def spreads(col):
    """({k: (d_at, d_rev, d_seq)} of x, the same of r.r); a large column's are kept though its arrays are not."""
    if col not in _SPREADS:
        column(col)
    return _SPREADS[col]


def bar(col, k):
    """The element-wise tolerance on x after k fixed loops, as a fraction of S_k."""
    return 100.0 * max(*spreads(col)[0][k], FLOOR)


def rr_bar(col, k):
    """The tolerance on the recurrence's r.r after k loops, as a fraction of T_k."""
    return 100.0 * max(*spreads(col)[1][k], FLOOR)


def all_columns(kind, n):
    return [Col(kind, n, j, z) for j in range(MAX_NRHS) for z in (False, True)]


def groups():
    """The table's rows: (label, columns)."""
    csr = sorted(set(CSR_SIZES) | {PLAN_CSR[0]})
    dense = sorted(set(DENSE_SIZES) | {PLAN_DENSE[0]})
    out = [(f"csr n={n}", all_columns("csr", n)) for n in csr]
    out += [(f"dense n={n}", all_columns("dense", n)) for n in dense]
    out.append((f"csr n={STRIDE[0]}", columns("csr", *STRIDE, "rough")))
    return out


def table():
    """The docstring's table, measured now."""
    rule = "=================  ========  ========  ========  ========  ========"
    lines = [rule, "cases              d_at      d_rev     d_seq     bar       rr bar", rule]
    for label, cols in groups():
        references(cols)
        worst = [max(spreads(c)[0][k][o] for c in cols for k in KS) for o in range(len(DOTS))]
        top = max(bar(c, k) for c in cols for k in KS)
        rr_top = max(rr_bar(c, k) for c in cols for k in rr_loops(c.n))
        lines.append(f"{label:<17s}  " + "  ".join(f"{v:.2e}" for v in worst) + f"  {top:.2e}  {rr_top:.2e}")
    return "\n".join(lines + [rule])


# ---- the lockstep fp64 restatement of a whole case, with the mutations of tests/test_nrhs_probe_cpu.py ---------------
MUTATIONS = ("neighbour alpha", "odd tail of p", "column pitch", "A x0 skipped", "beta one slot late", "pad column b")


def restate_case(kind, n, nrhs, variant, mutation=None, dot=None):
    """x after each of the loops 1..3, as (3, nrhs, n), of the fp64 restatement of every column of a case side by
    side; `mutation`: one of MUTATIONS, a wrong library restated."""
    assert mutation is None or mutation in MUTATIONS
    dot = dot or DOTS["d_at"]
    op = operator(kind, n)
    B, X0 = rhs(columns(kind, n, nrhs, variant))
    B, X0 = B.copy(), X0.copy()
    if mutation == "pad column b":  # the stored column nrhs - 1 takes what the pad columns read, column 0
        B[nrhs - 1] = B[0]
    if mutation == "column pitch":  # column j starts one column further on
        X0[:-1] = X0[1:].copy()
    x = X0
    r = np.stack([B[j] - (0.0 if mutation == "A x0 skipped" else op.apply(x[j])) for j in range(nrhs)])
    p = r.copy()
    rr = [dot(r[j], r[j]) for j in range(nrhs)]
    rr_old = list(rr)  # the ring slot before the current one
    out = []
    for _ in KS:
        Ap = [op.apply(p[j]) for j in range(nrhs)]
        alpha = [_ratio(rr[j], dot(p[j], Ap[j])) for j in range(nrhs)]
        if mutation == "neighbour alpha":
            alpha = alpha[:1] + alpha[:-1]
        x = np.stack([x[j] + alpha[j] * p[j] for j in range(nrhs)])
        r = np.stack([r[j] - alpha[j] * Ap[j] for j in range(nrhs)])
        rr_new = [dot(r[j], r[j]) for j in range(nrhs)]
        if mutation == "beta one slot late":
            beta = [_ratio(rr[j], rr_old[j]) for j in range(nrhs)]
        else:
            beta = [_ratio(rr_new[j], rr[j]) for j in range(nrhs)]
        p_new = np.stack([r[j] + beta[j] * p[j] for j in range(nrhs)])
        if mutation == "odd tail of p" and n % 2:
            p_new[:, -1] = p[:, -1]
        p, rr_old, rr = p_new, rr, rr_new
        out.append(x)
    return np.stack(out)


# ---- the freeze case ----------------------------------------------------------------------------------------------
FREEZE_PATTERNS = ([("odd", k) for k in (2, 4, 5, 8)] + [("even", k) for k in (2, 4, 5, 8)]
                   + [("all", 8), ("all", 1)])  # (pattern, nrhs)


def scaled_columns(pattern, nrhs):
    """The columns whose b and x0 are scaled by FREEZE_SCALE."""
    pick = {"odd": lambda j: j % 2 == 1, "even": lambda j: j % 2 == 0, "all": lambda j: True}[pattern]
    return [j for j in range(nrhs) if pick(j)]


def freeze_conditions(kind, n):
    """Asserted on the reference alone: a scaled column is at most FREEZE_EPS / 3 after loop 1, an unscaled one at
    least 3 FREEZE_EPS through loop 3.  Returns the two extremes."""
    refs = references(all_columns(kind, n))
    most = max(float(np.sqrt(ref.RR[1])) * FREEZE_SCALE for ref in refs)
    least = min(float(np.sqrt(ref.RR[k])) for ref in refs for k in RRKS)
    assert most <= FREEZE_EPS / 3 and least >= 3 * FREEZE_EPS, (kind, n, most, least)
    return most, least
