"""The CPU statement of block-Jacobi preconditioned CG as cgx_set_precond_block runs it (include/cgx.h, "Sparse A"),
and the block-scaled systems its tests solve.  numpy only.

The iteration is _pcg_ref.pcg's with z = W r applied block by block: from x0 = 0, r = b, p = z, then per loop
    alpha = r.z / p.Ap;  r -= alpha Ap;  x += alpha p;  stop when sqrt(r.r) < eps (r, not z, before the p update);
    z = W r;  beta = r.z_new / r.z_old;  p = z + beta p.
Block k covers rows [k bs, min(n, (k + 1) bs)); the reference's W_k is np.linalg.inv of A's k-th diagonal block -- it
does not go through the library's Cholesky inverse.

Systems: a base system (A, b) -- _pcg_ref.masked_base(n, seed), or oracle.poisson_dense(m) with b = 1 -- coupled
inside every block of bs rows:
    A' = S A S^T,  b' = S b,  S block lower-triangular on the bs grid: S[i][i] = h_i, S[i][j] = 0.5 h_i for j < i in
    the same block, h = sqrt(_pcg_ref.scaling(n, dec)).
(S A S^T is symmetrised, (M + M^T) / 2, so that A' is symmetric bit for bit.)  A diagonal scaling cannot undo S:
point Jacobi needs two to five times block Jacobi's loops on these systems and plain CG hundreds to thousands.

TABLE, measured with this file at eps = 1e-10: block-Jacobi loops, the ratio sqrt(r.r) / eps one iteration before
the stop and at it, and point Jacobi's loops.  A loop count is asserted only where the reference alone stands a
factor of 3 from the threshold on both sides (_pcg_ref.checked_reference's rule, `checked` below); every case of the
table does.  The three large masked systems carry every block size 2 .. 8, so every instantiation of the block
kernels solves a system of more than one thread block, with a short last block at n = 2101 and (but for bs = 7, which
divides it) at n = 1001; tests/_pcg_probe.py has every short block at every bs.  The n = 5 systems carry bs in
{2, 3, 4, 8}, the Poisson systems bs = 2.  Not to be used, they do not keep the factor: masked (1001, 2) and
(1000, 2) at dec 2 (ratio at ~ 0.9), masked (2101, 8) at dec 4 (0.85 - 0.98), Poisson m = 7 and m = 12 at every bs
tried, Poisson m = 5 at bs 3, 4, 8.  The largest condition number of a diagonal block among the cases is 2.3e4."""
import functools

import numpy as np

import _pcg_ref as pr
import oracle

EPS, TOL, MARGIN = pr.EPS, pr.TOL, pr.MARGIN

# (kind, size, seed or None, dec, bs): block loops, ratio before, ratio at, Jacobi loops
TABLE = {}


def _rows(kind, size, seed, dec, entries):
    for bs, row in entries.items():
        TABLE[(kind, size, seed, dec, bs)] = row


def nblocks(n, bs):
    return (n + bs - 1) // bs


def block_scaling(n, bs, dec):
    """S: block lower-triangular on the bs grid."""
    h = np.sqrt(pr.scaling(n, dec))
    i, j = np.indices((n, n))
    same = (i // bs) == (j // bs)
    return np.where(i == j, h[:, None], np.where(same & (j < i), 0.5 * h[:, None], 0.0))


def block_scale_system(A, b, bs, dec):
    S = block_scaling(b.size, bs, dec)
    M = S @ A @ S.T
    return pr.frozen(0.5 * (M + M.T), S @ b)


def diag_blocks(A, bs):
    """(nblk, bs, bs): A's diagonal blocks; the unused rows and columns of a short last block are +0.0."""
    n = A.shape[0]
    D = np.zeros((nblocks(n, bs), bs, bs))
    for k in range(D.shape[0]):
        lo, hi = k * bs, min(n, (k + 1) * bs)
        D[k, :hi - lo, :hi - lo] = A[lo:hi, lo:hi]
    return D


def inverse_blocks(A, bs):
    """The reference's W: np.linalg.inv of every diagonal block, in diag_blocks' layout."""
    n = A.shape[0]
    W = np.zeros((nblocks(n, bs), bs, bs))
    for k in range(W.shape[0]):
        lo, hi = k * bs, min(n, (k + 1) * bs)
        W[k, :hi - lo, :hi - lo] = np.linalg.inv(A[lo:hi, lo:hi])
    return W


def apply_blocks(W, r):
    """z = W r block by block."""
    nblk, bs, _ = W.shape
    rp = np.zeros(nblk * bs)
    rp[:r.size] = r
    return np.einsum("kij,kj->ki", W, rp.reshape(nblk, bs)).reshape(-1)[:r.size]


def pcg(A, b, apply, eps=EPS, max_iter=None):
    """(x, loops, converged, [r.r before the first loop, after loop 1, ...]) with z = apply(r); apply = None: plain
    CG.  eps < 0: max_iter loops, no stop."""
    ident = (lambda r: r)
    apply = apply or ident
    n = b.size
    cap = n if max_iter is None else max_iter
    x = np.zeros(n)
    r = np.array(b, np.float64)
    z = apply(r)
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
        z = apply(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, loops, conv, hist


def block_apply(W):
    return lambda r: apply_blocks(W, r)


def diag_apply(minv):
    return lambda r: minv * r


def checked(A, b, apply, margin=MARGIN, require=True, max_iter=None):
    """_pcg_ref.checked_reference's rule: (x, loops, ratio before, ratio at); loops is asserted (require) or None
    where the reference does not stand a factor of `margin` from the threshold on both sides."""
    x, K, conv, hist = pcg(A, b, apply, max_iter=max_iter)
    before, at = np.sqrt(hist[K - 1]) / EPS, np.sqrt(hist[K]) / EPS
    keeps = conv == 1 and at <= 1.0 / margin and before >= margin
    if require:
        assert keeps, (b.size, K, conv, before, at)
    return x, (K if keeps else None), before, at


def base_system(kind, size, seed):
    if kind == "masked":
        return pr.masked_base(size, seed)
    assert kind == "poisson" and seed is None
    return pr.frozen(oracle.poisson_dense(size), np.ones(size * size))


@functools.lru_cache(maxsize=None)
def system(kind, size, seed, dec, bs):
    """(A', its CSR, b', the reference's W, reference x, reference loops) of a case of TABLE."""
    A, b = block_scale_system(*base_system(kind, size, seed), bs, dec)
    W = pr.frozen(inverse_blocks(A, bs))[0]
    x, K, _, _ = checked(A, b, block_apply(W))
    return A, pr.to_csr(A), b, W, pr.frozen(x)[0], K


def jacobi_loops(A, b, max_iter=None):
    """(loops, converged, sqrt(r.r) at the end) of point-Jacobi PCG on the same system."""
    _, K, conv, hist = pcg(A, b, diag_apply(1.0 / np.diag(A)), max_iter=max_iter)
    return K, conv, np.sqrt(hist[K])


_rows("masked", 1001, 2, 4, {2: (7, 6.51, 0.040, 13), 3: (7, 6.40, 0.039, 18), 4: (7, 6.43, 0.040, 21),
                             5: (7, 6.28, 0.037, 24), 6: (7, 6.59, 0.039, 29), 7: (7, 7.14, 0.038, 30),
                             8: (7, 6.73, 0.039, 35)})
_rows("masked", 1000, 2, 4, {2: (7, 6.05, 0.036, 12), 3: (7, 6.00, 0.035, 17), 4: (7, 6.05, 0.035, 20),
                             5: (7, 6.19, 0.034, 24), 6: (7, 6.23, 0.035, 29), 7: (7, 6.57, 0.032, 33),
                             8: (7, 6.80, 0.034, 35)})
_rows("masked", 2101, 8, 2, {2: (6, 45.6, 0.122, 12), 3: (6, 45.5, 0.118, 16), 4: (6, 47.7, 0.120, 19),
                             5: (6, 52.1, 0.133, 22), 6: (6, 52.5, 0.131, 26), 7: (6, 54.0, 0.129, 29),
                             8: (6, 54.9, 0.138, 34)})
# n = 5: bs = 8 is n < bs, one short block, M = A, one loop
_rows("masked", 5, 3, 2, {2: (5, 1.7e6, 1.1e-7, 5), 3: (5, 2.0e6, 1.4e-8, 5), 4: (3, 4.9e8, 5.7e-7, 5),
                          8: (1, 1.1e11, 2.3e-5, 5)})
_rows("masked", 5, 3, 4, {2: (5, 9.7e6, 3.0e-7, 5), 3: (5, 1.1e7, 3.8e-7, 5), 4: (3, 2.0e9, 8.3e-6, 5),
                          8: (1, 5.9e11, 1.5e-4, 5)})
_rows("poisson", 5, None, 2, {2: (13, 2.1e3, 9.0e-7, 24)})
_rows("poisson", 5, None, 4, {2: (13, 1.2e4, 3.2e-5, 24)})
