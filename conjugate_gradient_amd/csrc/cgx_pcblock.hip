// cgx_pcblock.hip -- the host side of block-Jacobi preconditioning (cgx.h,
// "Sparse A"): the inversion of A's diagonal blocks and the check of a
// caller's inverse blocks.  Plain C++, no device code, no GPU needed.
//
// Layout of D and W: nblk = ceil(n / bs) blocks of bs * bs doubles, block after
// block, row-major inside a block; a short last block (t = n % bs rows) uses
// its leading t x t entries, the rest is +0.0 on output and ignored on input.
//
// Contraction is off for this translation unit (the pragma below, and the
// Makefile's -ffp-contract=off), so every product and sum here rounds once:
// the same blocks give the same bits under any optimisation level.
#include <cmath>
#include <cstdint>

#include "cgx.h"

#pragma clang fp contract(off)

namespace cgxh {
int fail(int code, const char *fmt, ...);
}
using cgxh::fail;

namespace {

constexpr int kB = CGX_MAX_PC_BLOCK;

int check_shape(const char *fn, int64_t n, int bs) {
    if (n < 1) return fail(CGX_ERR_ARG, "%s: n must be >= 1", fn);
    if (bs == 1) return fail(CGX_ERR_ARG, "%s: bs = 1 is point Jacobi: use CGX_PC_JACOBI (cgx_set_precond)", fn);
    if (bs < 2 || bs > kB) return fail(CGX_ERR_ARG, "%s: bs must be in [2, %d] (got %d)", fn, kB, bs);
    return CGX_OK;
}

// W = (L L^T)^-1 of the leading t x t part of D (row pitch bs), reading D's
// lower triangle only.  Returns -1, or the index of the first pivot that is
// not finite or not > 0 (its value in *pivot).
int invert_block(int t, int bs, const double *D, double *W, double *pivot) {
    double L[kB][kB], Li[kB][kB];
    for (int j = 0; j < t; ++j) {  // Cholesky, column by column
        double s = D[j * bs + j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(std::isfinite(s) && s > 0.0)) {
            *pivot = s;
            return j;
        }
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < t; ++i) {
            double v = D[i * bs + j];
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    for (int j = 0; j < t; ++j) {  // Li = L^-1 (lower), column by column
        Li[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < t; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v = v - L[i][k] * Li[k][j];
            Li[i][j] = v / L[i][i];
        }
    }
    for (int i = 0; i < t; ++i)  // W = Li^T Li: the lower triangle, mirrored
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = i; k < t; ++k) v = v + Li[k][i] * Li[k][j];
            W[i * bs + j] = v;
            W[j * bs + i] = v;
        }
    return -1;
}

}  // namespace

extern "C" {

int cgx_precond_block_invert(int64_t n, int bs, const double *D, double *W) {
    if (int rc = check_shape("cgx_precond_block_invert", n, bs)) return rc;
    if (!D || !W) return fail(CGX_ERR_ARG, "cgx_precond_block_invert: NULL pointer");
    const int64_t nblk = (n + bs - 1) / bs;
    for (int64_t k = 0; k < nblk; ++k) {
        const int64_t row0 = k * bs;
        const int t = (int)(n - row0 < bs ? n - row0 : bs);
        double *Wk = W + k * bs * bs;
        for (int e = 0; e < bs * bs; ++e) Wk[e] = 0.0;
        double pivot = 0.0;
        const int j = invert_block(t, bs, D + k * bs * bs, Wk, &pivot);
        if (j >= 0)
            return fail(CGX_ERR_SHAPE,
                        "cgx_precond_block_invert: block %lld (rows %lld..%lld): pivot %d = %.17g is not finite or "
                        "not > 0 (the diagonal block is not positive definite)",
                        (long long)k, (long long)row0, (long long)(row0 + t - 1), j, pivot);
    }
    return CGX_OK;
}

int cgx_precond_block_check(int64_t n, int bs, const double *W) {
    if (int rc = check_shape("cgx_precond_block_check", n, bs)) return rc;
    if (!W) return fail(CGX_ERR_ARG, "cgx_precond_block_check: NULL pointer");
    const int64_t nblk = (n + bs - 1) / bs;
    for (int64_t k = 0; k < nblk; ++k) {
        const int64_t row0 = k * bs;
        const int t = (int)(n - row0 < bs ? n - row0 : bs);
        for (int i = 0; i < t; ++i)
            for (int j = 0; j < t; ++j) {
                const double w = W[k * bs * bs + i * bs + j];
                if (!std::isfinite(w))
                    return fail(CGX_ERR_SHAPE, "cgx_precond_block_check: W[%lld][%d][%d] = %.17g is not finite",
                                (long long)k, i, j, w);
                if (i == j && !(w > 0.0))
                    return fail(CGX_ERR_SHAPE,
                                "cgx_precond_block_check: W[%lld][%d][%d] = %.17g, a diagonal entry, is not > 0",
                                (long long)k, i, j, w);
            }
    }
    return CGX_OK;
}

}  // extern "C"
