"""Extended-precision reference and probe data for the preconditioned CG kernels of CSR contexts (cgx_pcg.hip,
cgx_pcg_block.hip).

numpy only -- none of it is the code under test.  Cached arrays are read-only.  The module refuses to load where long
double has no more bits than double: a comparison of fp64 with fp64 would say nothing about either.

The probe: three fixed loops (eps = -1) of preconditioned CG from a rough x0 on a rough b with an unsymmetric W, x read
after each loop.  x_1 = x_0 + alpha_0 W r_0 shows the start kernel's z row by row; x_2 - x_1 = alpha_1 (W r_1 +
beta_1 W r_0) and x_3 show the z that the r update stores and the x/p update's read of it.

``system(n)``: A symmetric and banded, held as its bands: diagonal 4 + u_i (u in [0, 1)), bands at distances 1, 2
and 37 with values in [-0.5, 0.5) -- every row's off-diagonal entries sum to less than 3 in magnitude, so A is strictly
diagonally dominant, hence SPD; the 37-band couples different blocks at every bs.  ``System.apply`` is the operator
by shifted slices in the argument's type, ``System.csr`` the same matrix as CSR arrays (columns ascending).  b and x0
are seeded in [-0.5, 0.5), both nonzero; the ``zero`` variant of a case starts from x0 = 0 (the start that skips
A x0).

``blocks(n, bs)``: W of shape (nblk, bs, bs), diagonal in [0.5, 2), off-diagonal in [-0.4 / bs, 0.4 / bs), not
symmetric.  By Gershgorin the symmetric part of every block is at least 0.1 I, so r.z = r^T sym(W) r >= 0.1 r.r > 0
and p.Ap > 0 on the reference alone (asserted at every loop).  It returns two arrays: the reference's, with zeros
outside the leading t x t of a short last block, and the one handed to the library, with NaN there (the header:
"ignored on input").  ``minv(n, kind)``: seeded in [0.5, 2) for "diag", 1 / diag(A) for "jacobi".

``probe(case)``: x_ld after each of the loops 1..3 in np.longdouble (a sequential statement of the recurrence of
tests/_bpcg_ref.py, not the kernels' order; alpha and beta by the library's rule that 0 / 0 is 0, which only an exactly
solved system reaches) and the per-element scale
    S_k[i] = |x0_i| + sum_{m<k} |alpha_m| P_m[i],   P_0 = |W| |r_0|,   P_m = |W| |r_m| + |beta_m| P_(m-1),
the magnitude of every term that was added into x_i.  A global max|x| would hide a wrong row of small magnitude, such
as one of the short block.

``bar(case, k)``: the element-wise tolerance of tests/test_gpu_pcg_probe.py, |x[i] - x_ld[i]| <= bar S_k[i] for every
i: this suite's rule (tests/_long_systems.py, tests/_poisson_probe.py), 100 x the measured spread between fp64
summation orders.  The spread is the largest |x_f64 - x_ld| / S over three fp64 restatements of the recurrence that
differ only in their dots: numpy's ``@``, ``@`` on the reversed vectors, and the strictly sequential ``cumsum``;
floored at FLOOR = 4 ulp of fp64 (8.9e-16: the cases of at most 7 rows measure 0.2 to 1.7 ulp and the cases of 255 to
4097 rows 3.2 to 31 ulp, so the floor lies between them and lifts only what measures less).  The kernels' order is a
fourth one.

Measured (printed by ``pytest -s tests/test_pcg_probe_cpu.py``, which asserts every bar <= 1e-10).  A row is the worst
of its group over the x0 variants (rough and 0), the loops k = 1..3 and, for the blocks, every t = n % bs:

=============================  ========  ========  ========  ========
cases                          d_at      d_rev     d_seq     bar
=============================  ========  ========  ========  ========
block bs=2, n=257 bs+t         4.48e-16  2.81e-15  2.05e-15  2.81e-13
block bs=3, n=257 bs+t         5.82e-16  2.33e-15  1.24e-15  2.33e-13
block bs=4, n=257 bs+t         8.23e-16  2.81e-15  2.22e-15  2.81e-13
block bs=5, n=257 bs+t         8.57e-16  3.41e-15  3.04e-15  3.41e-13
block bs=6, n=257 bs+t         8.24e-16  3.58e-15  2.61e-15  3.58e-13
block bs=7, n=257 bs+t         7.79e-16  2.72e-15  3.17e-15  3.17e-13
block bs=8, n=257 bs+t         9.46e-16  4.05e-15  3.49e-15  4.05e-13
block bs=2, n=1                4.37e-17  4.37e-17  4.37e-17  8.88e-14
block bs=3, n=2                1.81e-16  1.81e-16  1.81e-16  8.88e-14
block bs=4, n=3                2.42e-16  2.42e-16  2.42e-16  8.88e-14
block bs=5, n=4                3.80e-16  1.77e-16  3.47e-16  8.88e-14
block bs=6, n=5                3.15e-16  1.79e-16  3.15e-16  8.88e-14
block bs=7, n=6                2.87e-16  2.04e-16  2.04e-16  8.88e-14
block bs=8, n=7                2.20e-16  3.21e-16  2.20e-16  8.88e-14
diag, jacobi n=1               9.08e-17  9.08e-17  9.08e-17  8.88e-14
diag, jacobi n=2               2.07e-16  1.83e-16  1.83e-16  8.88e-14
diag, jacobi n=3               3.21e-16  1.88e-16  3.21e-16  8.88e-14
diag, jacobi n=255             1.03e-15  1.90e-15  1.34e-15  1.90e-13
diag, jacobi n=256             1.40e-15  1.65e-15  9.95e-16  1.65e-13
diag, jacobi n=257             8.64e-16  1.05e-15  1.59e-15  1.59e-13
diag, jacobi n=2047            1.42e-15  2.94e-15  3.98e-15  3.98e-13
diag, jacobi n=2048            2.00e-15  3.75e-15  2.34e-15  3.75e-13
diag, jacobi n=2049            1.22e-15  3.38e-15  5.36e-15  5.36e-13
diag, jacobi n=4097            1.59e-15  6.89e-15  6.17e-15  6.89e-13
diag n=772                     1.54e-15  2.35e-15  2.01e-15  2.35e-13
diag n=2057                    1.06e-15  3.08e-15  1.26e-15  3.08e-13
block bs=2, n=1048579          3.55e-15  1.78e-14  7.68e-14  7.68e-12
diag n=4194307                 1.28e-14  1.39e-13  1.45e-13  1.45e-11
=============================  ========  ========  ========  ========

The mutations of tests/test_pcg_probe_cpu.py (W transposed, one entry zeroed, the short block one row short, minv
shifted by one element) move some element of x_1 by at least 6.9e-4 of S_1: 4e9 bars.
"""
import collections
import concurrent.futures
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, (
    f"np.longdouble has eps = {np.finfo(LD).eps:.3g} on this machine: no extended precision, the PCG probe "
    "reference would compare fp64 with fp64")

ULP = float(np.finfo(np.float64).eps)
FLOOR = 4 * ULP
CAP = 1e-10  # this suite's TOL: every bar stays under it
KS = (1, 2, 3)
DIST = (1, 2, 37)
SMALL = 1 << 16  # arrays of larger cases are not kept

# kind: "block" (bs in 2..8), "diag" or "jacobi" (bs = 0); zero: x0 = 0
Case = collections.namedtuple("Case", "kind bs n zero")

BLOCK_SIZES = tuple(range(2, 9))
BLOCK_CASES = tuple((bs, t) for bs in BLOCK_SIZES for t in range(bs))  # n = 257 bs + t: two thread blocks of blocks
DIAG_KINDS = ("diag", "jacobi")
DIAG_SIZES = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097)  # the pair loop's chunk of 1024 pairs, either side
DIAGONAL_BLOCK_SIZES = (3, 8)  # blocks with only the diagonal set, n = 257 bs + 1, against the "diag" reference
BLOCK_STRIDE = (2, 2 * 524288 + 3)  # (bs, n): nblk = 524290 > 2048 * 256, two blocks reached by the stride only
DIAG_STRIDE = 2 * 2048 * 1024 + 3  # pairs past 2048 blocks * 1024, and an odd tail


def block_n(bs, t):
    return 257 * bs + t


def nblocks(n, bs):
    return (n + bs - 1) // bs


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def _keep_small(fn):
    """functools.lru_cache for calls whose first argument (n, or a Case) is at most SMALL rows."""
    kept = {}

    @functools.wraps(fn)
    def wrapper(*args):
        if args in kept:
            return kept[args]
        out = fn(*args)
        if (args[0].n if isinstance(args[0], Case) else args[0]) <= SMALL:
            kept[args] = out
        return out
    return wrapper


class System:
    """The banded A of n rows, b and x0."""

    def __init__(self, n):
        rng = np.random.default_rng([n, 1])
        self.n, self._typed = n, {}
        self.diag = 4.0 + rng.random(n)
        self.off = {d: rng.random(max(n - d, 0)) - 0.5 for d in DIST}  # A[i, i + d] = A[i + d, i] = off[d][i]
        self.b = rng.random(n) - 0.5
        self.x0 = rng.random(n) - 0.5
        assert np.all(self.b != 0.0) and np.all(self.x0 != 0.0)
        _ro(self.diag, self.b, self.x0, *self.off.values())

    def apply(self, p):
        """A p by shifted slices, in p's own type."""
        if p.dtype not in self._typed:  # the bands in p's type, converted once
            self._typed[p.dtype] = (self.diag.astype(p.dtype), {d: c.astype(p.dtype) for d, c in self.off.items()})
        diag, off = self._typed[p.dtype]
        out = diag * p
        for d, c in off.items():
            if d < self.n:
                out[:-d] += c * p[d:]
                out[d:] += c * p[:-d]
        return out

    def csr(self):
        """(indptr, indices, data): the columns i - 37, i - 2, i - 1, i, i + 1, i + 2, i + 37 that exist, ascending."""
        n = self.n
        i = np.arange(n, dtype=np.int64)
        cols = np.zeros((n, 2 * len(DIST) + 1), np.int64)
        vals = np.zeros(cols.shape)
        have = np.zeros(cols.shape, bool)
        mid = len(DIST)
        cols[:, mid], vals[:, mid], have[:, mid] = i, self.diag, True
        for s, d in enumerate(DIST, 1):
            if d < n:
                cols[d:, mid - s], vals[d:, mid - s], have[d:, mid - s] = i[d:] - d, self.off[d], True
                cols[:n - d, mid + s], vals[:n - d, mid + s], have[:n - d, mid + s] = i[:n - d] + d, self.off[d], True
        indptr = np.concatenate([[0], np.cumsum(have.sum(axis=1))]).astype(np.int64)
        return indptr, cols[have].astype(np.int32), vals[have]

    def dense(self):
        """The explicit matrix, from the CSR arrays (small n)."""
        indptr, indices, data = self.csr()
        A = np.zeros((self.n, self.n))
        A[np.repeat(np.arange(self.n), np.diff(indptr)), indices] = data
        return A


@_keep_small
def system(n):
    return System(n)


@_keep_small
def blocks(n, bs):
    """(the reference's W, the W handed to the library): zeros / NaN outside the used t x t of a short last block."""
    nblk = nblocks(n, bs)
    rng = np.random.default_rng([n, bs, 2])
    W = (rng.random((nblk, bs, bs)) - 0.5) * (0.8 / bs)
    i = np.arange(bs)
    W[:, i, i] = 0.5 + 1.5 * rng.random((nblk, bs))
    t = n - (nblk - 1) * bs
    ref, given = W.copy(), W.copy()
    for arr, fill in ((ref, 0.0), (given, np.nan)):
        arr[-1, t:, :] = fill
        arr[-1, :, t:] = fill
    return _ro(ref, given)


@_keep_small
def minv(n, kind):
    if kind == "jacobi":
        return _ro(1.0 / system(n).diag)[0]
    assert kind == "diag"
    return _ro(0.5 + 1.5 * np.random.default_rng([n, 3]).random(n))[0]


def diagonal_blocks(n, bs):
    """(nblk, bs, bs) for the library: minv(n, "diag") on the diagonals, +0.0 beside them, NaN in the unused slots."""
    W = blocks(n, bs)[1].copy()
    W[np.isfinite(W)] = 0.0
    i = np.arange(n)
    W[i // bs, i % bs, i % bs] = minv(n, "diag")
    return W


def precond(case):
    """The reference's M^-1 in fp64: (nblk, bs, bs) blocks, or the n values of a diagonal kind."""
    return blocks(case.n, case.bs)[0] if case.kind == "block" else minv(case.n, case.kind)


def library_precond(case):
    """What the library is given: blocks with NaN in the unused slots, the values of "diag", or "jacobi"."""
    if case.kind == "block":
        return blocks(case.n, case.bs)[1]
    return "jacobi" if case.kind == "jacobi" else minv(case.n, "diag")


def apply_m(M, r):
    """z = M^-1 r in r's type; the blocks row by row, j ascending (the header's order, without the fusing)."""
    M = M.astype(r.dtype)
    if M.ndim == 1:
        return M * r
    nblk, bs, _ = M.shape
    R = np.zeros(nblk * bs, r.dtype)
    R[:r.size] = r
    R = R.reshape(nblk, bs)
    Z = np.empty_like(R)
    for i in range(bs):
        acc = M[:, i, 0] * R[:, 0]
        for j in range(1, bs):
            acc = acc + M[:, i, j] * R[:, j]
        Z[:, i] = acc
    return Z.reshape(-1)[:r.size]


def _ratio(num, den):
    """num / den; 0 where the system is solved exactly (0 / 0), as the kernels' cg_ratio."""
    return num / den if den != 0 or not abs(num) < 2.0 ** -1022 else num * 0


def pcg(sys_, x0, M, dtype, dot, scales=False):
    """x after each of the loops 1..max(KS) of preconditioned CG in `dtype` with the given dot, no stopping test;
    with `scales` also S_k, and r.z >= 0.1 r.r asserted at every loop."""
    b = sys_.b.astype(dtype)
    x = x0.astype(dtype)
    r = b - sys_.apply(x)
    z = apply_m(M, r)
    p = z.copy()
    rz = dot(r, z)
    X, S = [], []
    if scales:
        Mabs = np.abs(M)
        assert rz >= 0.1 * dot(r, r) > 0
        s, P = np.abs(x), apply_m(Mabs, np.abs(r))
    for _ in range(max(KS)):
        Ap = sys_.apply(p)
        alpha = _ratio(rz, dot(p, Ap))
        x = x + alpha * p
        r = r - alpha * Ap
        X.append(x)
        z = apply_m(M, r)
        rz_new = dot(r, z)
        beta = _ratio(rz_new, rz)
        if scales:
            assert alpha >= 0 and rz_new >= 0.1 * dot(r, r), (alpha, rz_new)
            s = s + abs(alpha) * P
            S.append(s)
            P = apply_m(Mabs, np.abs(r)) + abs(beta) * P
        p = z + beta * p
        rz = rz_new
    return (X, S) if scales else X


def _dot_ld(a, b):
    return np.dot(a, b)  # long double: numpy's plain loop, one element after the other


DOTS = collections.OrderedDict([
    ("d_at", lambda a, b: a @ b),  # numpy's @: the BLAS dot, blocked partial sums
    ("d_rev", lambda a, b: a[::-1] @ b[::-1]),  # the same on the reversed vectors
    ("d_seq", lambda a, b: np.cumsum(a * b)[-1]),  # strictly one element after the other
])


def start(case):
    """(system, x0) of a case."""
    sys_ = system(case.n)
    return sys_, (np.zeros(case.n) if case.zero else sys_.x0)


def restate(case, dot, M=None, at=None):
    """x after the loops 1..3 of an fp64 restatement; M: another preconditioner than the case's (the mutations);
    at: start(case), where the caller has it."""
    sys_, x0 = at or start(case)
    return pcg(sys_, x0, precond(case) if M is None else M, np.float64, dot)


def ratios(x, x_ld, S):
    """|x - x_ld| / S per element, formed in long double."""
    return np.abs(np.asarray(x, LD) - x_ld) / S


Probe = collections.namedtuple("Probe", "case X S spread")  # X, S: {k: array}; spread: {k: (d_at, d_rev, d_seq)}
_SPREADS = {}


@_keep_small
def probe(case):
    """The reference of a case: x_ld (long double) and S (fp64) after each loop, and the spreads of the three fp64
    orders against it."""
    sys_, x0 = start(case)
    for dtype in (LD, np.float64):
        sys_.apply(np.zeros(case.n, dtype))  # the typed bands, before the threads read them
    # the four runs are independent; side by side a million rows take the long-double run's time
    with concurrent.futures.ThreadPoolExecutor(1 + len(DOTS)) as pool:
        M = precond(case)
        ld = pool.submit(pcg, sys_, x0, M, LD, _dot_ld, True)
        f64 = [pool.submit(restate, case, dot, M, (sys_, x0)) for dot in DOTS.values()]
        X, S = ld.result()
        f64 = [f.result() for f in f64]
    assert all(np.all(s > 0) for s in S)
    spread = {k: [] for k in KS}
    for Xf in f64:
        for k in KS:
            spread[k].append(float(np.max(ratios(Xf[k - 1], X[k - 1], S[k - 1]))))
    _SPREADS[case] = {k: tuple(v) for k, v in spread.items()}
    return Probe(case, {k: _ro(X[k - 1])[0] for k in KS}, {k: _ro(S[k - 1].astype(np.float64))[0] for k in KS},
                 _SPREADS[case])


def spreads(case):
    """{k: (d_at, d_rev, d_seq)}; a large case's are kept though its arrays are not."""
    return _SPREADS[case] if case in _SPREADS else probe(case).spread


def bar(case, k):
    """The element-wise tolerance after k fixed loops, as a fraction of S_k."""
    return 100.0 * max(*spreads(case)[k], FLOOR)


def block_case(bs, t, zero=False):
    return Case("block", bs, block_n(bs, t), zero)


def groups():
    """The table's rows: (label, cases)."""
    both = (False, True)
    out = [(f"block bs={bs}, n=257 bs+t", [block_case(bs, t, z) for t in range(bs) for z in both])
           for bs in BLOCK_SIZES]
    out += [(f"block bs={bs}, n={bs - 1}", [Case("block", bs, bs - 1, z) for z in both]) for bs in BLOCK_SIZES]
    out += [(f"diag, jacobi n={n}", [Case(kind, 0, n, z) for kind in DIAG_KINDS for z in both]) for n in DIAG_SIZES]
    out += [(f"diag n={block_n(bs, 1)}", [Case("diag", 0, block_n(bs, 1), z) for z in both])
            for bs in DIAGONAL_BLOCK_SIZES]
    out += [(f"block bs={BLOCK_STRIDE[0]}, n={BLOCK_STRIDE[1]}", [Case("block", *BLOCK_STRIDE, False)]),  # x0 rough only
            (f"diag n={DIAG_STRIDE}", [Case("diag", 0, DIAG_STRIDE, False)])]
    return out


def all_cases():
    return [c for _, cases in groups() for c in cases]


def table():
    """The docstring's table, measured now."""
    rule = "=============================  ========  ========  ========  ========"
    lines = [rule, "cases                          d_at      d_rev     d_seq     bar", rule]
    for label, cases in groups():
        worst = [max(spreads(c)[k][o] for c in cases for k in KS) for o in range(len(DOTS))]
        top = max(bar(c, k) for c in cases for k in KS)
        lines.append(f"{label:<29s}  " + "  ".join(f"{v:.2e}" for v in worst) + f"  {top:.2e}")
    return "\n".join(lines + [rule])
