"""The CPU statement of diagonally preconditioned CG as cgx_set_precond runs it (include/cgx.h, "Sparse A"), and the
scaled systems its tests solve.  numpy only.

The iteration, from x0 = 0: r = b, p = z = minv o r, then per loop
    alpha = r.z / p.Ap;  r -= alpha Ap;  x += alpha p;  stop when sqrt(r.r) < eps (r, not z, before the p update);
    z = minv o r (a rounded product);  beta = r.z_new / r.z_old;  p = z + beta p.

Scaled systems: from a base system (A, b) -- the masked systems of test_gpu_csr.py (mask, to_csr, oracle.spd_hash)
or the 5-point Poisson matrix with b = 1 everywhere -- with d_i = 10 ** (dec * ((i * 7919) mod n) / n):
    A' = D^(1/2) A D^(1/2),   b' = s * D^(1/2) b.
Plain CG needs thousands of loops on them, Jacobi-PCG a handful (TABLE below, measured with this file at eps = 1e-10:
the Jacobi loop count, the ratio sqrt(r.r) / eps one iteration before the stop and at it, and plain CG's loop count
with the cap lifted to 12000 loops; None: not converged after 3000 loops.  Plain CG's count in the thousands moves
with the last bits of the dots, so it is a figure, not a contract: test_pcg_cpu.py holds it to 2 %, and runs it only
where n <= 1001).  A Jacobi loop count is asserted only where the reference alone stands a factor of 3 from the
threshold on both sides (checked_reference, test_gpu_csr.py's rule); the cases are chosen so that it does.  Not to be
used, they do not keep the factor: masked (130, 5, 4, 1), (1000, 2, 4, 1e-3), (1001, 2, 6, 1), (5001, 9, 6, 1) and
Poisson (16, 4, 1), (16, 4, 2)."""
import functools

import numpy as np

import oracle

EPS = 1e-10
TOL = 1e-10
MARGIN = 3.0

# (n, seed, dec, s): Jacobi loops, ratio before, ratio at, plain CG loops
MASKED_TABLE = {
    (1, 3, 0, 1.0): (1, None, 1.1e-6, 1),
    (5, 3, 3, 1.0): (5, 2.5e6, 4.8e-8, 6),
    (1001, 2, 4, 1.0): (7, 6.70, 0.042, 1247),
    (1000, 2, 6, 1.0): (7, 49.3, 0.281, 10976),
    (2101, 8, 6, 1.0): (7, 6.47, 0.020, None),
    (5001, 9, 4, 1.0): (6, 85.7, 0.147, 1415),
}
# (m, dec, s)
POISSON_TABLE = {
    (5, 3, 1.0): (5, 1.4e10, 4.2e-5, 43),
    (7, 4, 1.0): (9, 1.5e9, 1.4e-4, 154),
    (12, 4, 1.0): (21, 1.2e4, 1.7e-3, 735),
    (16, 6, 1.0): (34, 4.26, 0.147, None),
}


def frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def mask(n):
    """test_gpu_csr.py's sparsity pattern."""
    i, j = np.indices((n, n))
    d = np.abs(i - j)
    return (d <= 2) | (((i + j) % 7 == 0) & (d <= 64)) | (i % 50 == 0) | (j % 50 == 0)


def to_csr(A):
    """(indptr, indices, data) of the entries of A that are not 0, row by row in column order."""
    rows, cols = np.nonzero(A)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))]).astype(np.int64)
    return frozen(indptr, cols.astype(np.int32), np.ascontiguousarray(A[rows, cols]))


def scaling(n, dec):
    i = np.arange(n, dtype=np.int64)
    return 10.0 ** (dec * ((i * 7919) % n) / n)


def scale_system(A, b, dec, s):
    """(A', b') = (D^(1/2) A D^(1/2), s D^(1/2) b)."""
    h = np.sqrt(scaling(b.size, dec))
    return frozen(h[:, None] * A * h[None, :], s * (h * b))


def pcg(A, b, minv, eps=EPS, max_iter=None):
    """(x, loops, converged, [r.r before the first loop, after loop 1, ...]); minv = None: plain CG.
    eps < 0: max_iter loops, no stop."""
    n = b.size
    cap = n if max_iter is None else max_iter
    x = np.zeros(n)
    r = np.array(b, np.float64)
    z = r if minv is None else minv * r
    p = z.copy()
    rz = r @ z
    hist = [r @ r]
    loops, conv = 0, 0
    for _ in range(cap):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        r = r - alpha * Ap
        x = x + alpha * p
        rr = r @ r
        hist.append(rr)
        loops += 1
        if eps >= 0.0 and np.sqrt(rr) < eps:
            conv = 1
            break
        z = r if minv is None else minv * r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, loops, conv, hist


def checked_reference(A, b, minv, margin=MARGIN, require=True):
    """(x, loops, ratio before, ratio at) of pcg from x0 = 0.  require: the factor-of-`margin` distance from the
    threshold on both sides is asserted; otherwise loops is None where the reference does not keep it."""
    x, K, conv, hist = pcg(A, b, minv)
    before, at = np.sqrt(hist[K - 1]) / EPS, np.sqrt(hist[K]) / EPS
    keeps = conv == 1 and at <= 1.0 / margin and before >= margin
    if require:
        assert keeps, (b.size, K, conv, before, at)
    return x, (K if keeps else None), before, at


@functools.lru_cache(maxsize=2)
def masked_base(n, seed):
    A, b = oracle.spd_hash(n, seed=seed)
    return frozen(A * mask(n), b)


@functools.lru_cache(maxsize=None)
def masked_system(n, seed, dec, s):
    """(A', its CSR, b', minv = 1 / diag(A'), reference x, reference loops) of a masked case of MASKED_TABLE."""
    A, b = scale_system(*masked_base(n, seed), dec, s)
    minv = frozen(1.0 / np.diag(A))[0]
    x, K, _, _ = checked_reference(A, b, minv)
    return A, to_csr(A), b, minv, frozen(x)[0], K


@functools.lru_cache(maxsize=None)
def poisson_system(m, dec, s):
    """The same for a Poisson case of POISSON_TABLE (b = 1 everywhere before the scaling)."""
    A, b = scale_system(oracle.poisson_dense(m), np.ones(m * m), dec, s)
    minv = frozen(1.0 / np.diag(A))[0]
    x, K, _, _ = checked_reference(A, b, minv)
    return A, to_csr(A), b, minv, frozen(x)[0], K
