// cgx_pcg_block.hip -- block-Jacobi preconditioned CG on cgx_create_csr contexts
// (cgx_set_precond_block / cgx_set_precond_block_values, cgx_csr.hip): the start
// of the solve and the two update kernels with z = W r applied block by block,
// and the one-time extraction of A's bs x bs diagonal blocks from the CSR arrays.
//
// Block k covers rows [k bs, min(n, (k + 1) bs)); W holds the nblk = ceil(n / bs)
// inverse blocks.  On the device entry (i, j) of block k lives at
// W[(i * BS + j) * wld + k] (wld >= nblk): one thread owns one block, so the 64
// lanes of a wave read 64 consecutive doubles per entry.  The new r of a block
// is in the owning thread's registers when z is formed; W is streamed row by
// row (BS loads per z_i), never held whole.
//
// Unlike the diagonal kinds (cgx_pcg.hip) z is stored: recomputing it in the
// x/p kernel would read W again (16 BS bytes per row against 16 for the write
// and the read of z).  So the x/p kernel is element-wise and needs no BS.
// Per row and iteration: r update 32 + 8 BS bytes, x/p update 40.
//
// Contraction contract.  Contraction is off and the fused operations are
// spelled out, with j over the block's rows in ascending order:
//   r_i   = fma(-alpha, Ap_i, r_i)
//   z_i   = fl(W[i][0] r_0), then z_i = fma(W[i][j], r_j, z_i) for j = 1, ...
//   x_i   = fma(alpha, p_i, x_i),  p_i = fma(beta, p_i, z_i)
//   dots  : acc = fma(r_i, r_i, acc) and acc = fma(r_i, z_i, acc), a thread's
//           rows in ascending order, then grid_sum_last_block_n<2> -- fixed for
//           a given (n, BS); not the diagonal kernels' order.
// The short last block (t = n % BS rows) uses its leading t x t entries only.
#include "cgx_vector_core.h"

namespace cgx {
namespace {

// rows [0, BS) of a block at p (FULL), or its first t rows (the rest +0.0)
template <int BS, bool FULL, bool NT>
__device__ __forceinline__ void ld_blk(const double *__restrict__ p, int t, double (&v)[BS]) {
    if constexpr (FULL && BS % 2 == 0) {  // row0 = k BS is even: 16-byte loads
#pragma unroll
        for (int i = 0; i < BS; i += 2) {
            const d2 w = NT ? ldv<2>(p + i) : ld2(p + i);
            v[i] = w.x;
            v[i + 1] = w.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            if (FULL || i < t) v[i] = NT ? __builtin_nontemporal_load(p + i) : p[i];
            else v[i] = 0.0;
        }
    }
}

template <int BS, bool FULL, bool NT>
__device__ __forceinline__ void st_blk(double *__restrict__ p, int t, const double (&v)[BS]) {
    if constexpr (FULL && BS % 2 == 0) {
#pragma unroll
        for (int i = 0; i < BS; i += 2) {
            d2 w;
            w.x = v[i];
            w.y = v[i + 1];
            if (NT) stv<2>(p + i, w);
            else st2(p + i, w);
        }
    } else {
#pragma unroll
        for (int i = 0; i < BS; ++i)
            if (FULL || i < t) {
                if (NT) __builtin_nontemporal_store(v[i], p + i);
                else p[i] = v[i];
            }
    }
}

// z = W_k r in the header's order; both dots take the block's rows in order
template <int BS, bool FULL>
__device__ __forceinline__ void apply_w(const double *__restrict__ W, int64_t wld, int64_t k, int t,
                                        const double (&r)[BS], double (&z)[BS], double (&acc)[2]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < BS; ++i) {
        z[i] = 0.0;
        if (FULL || i < t) {
            const double *w = W + (int64_t)(i * BS) * wld + k;
            double zi = w[0] * r[0];
#pragma unroll
            for (int j = 1; j < BS; ++j)
                if (FULL || j < t) zi = __builtin_fma(w[(int64_t)j * wld], r[j], zi);
            z[i] = zi;
            acc[0] = __builtin_fma(r[i], r[i], acc[0]);
            acc[1] = __builtin_fma(r[i], zi, acc[1]);
        }
    }
}

// r = b - A x (Ax == nullptr: b - 0.0), p = z = W r, out[0] = r.r,
// out[stride] = r.z; block 0 resets the convergence record (k_pcg_residual_f64).
// z itself is not stored: the first r update writes it before anything reads it.
template <int BS>
__global__ __launch_bounds__(kNT) void k_pcgb_residual_f64(int64_t n, int64_t nblk, const double *__restrict__ b,
                                                           const double *__restrict__ Ax,
                                                           const double *__restrict__ W, int64_t wld,
                                                           double *__restrict__ r, double *__restrict__ p, double *out,
                                                           int stride, double *partials, unsigned *ticket,
                                                           int64_t *clear2) {
#pragma clang fp contract(off)
    if (clear2 && blockIdx.x == 0 && threadIdx.x < 2) clear2[threadIdx.x] = 0;
    double acc[2] = {0.0, 0.0};
    for (int64_t k = (int64_t)blockIdx.x * kNT + threadIdx.x; k < nblk; k += (int64_t)gridDim.x * kNT) {
        const int64_t row0 = k * BS;
        double bv[BS], av[BS], rv[BS], zv[BS];
        if (n - row0 >= BS) {
            ld_blk<BS, true, false>(b + row0, BS, bv);
            if (Ax) ld_blk<BS, true, false>(Ax + row0, BS, av);
#pragma unroll
            for (int i = 0; i < BS; ++i) rv[i] = bv[i] - (Ax ? av[i] : 0.0);
            apply_w<BS, true>(W, wld, k, BS, rv, zv, acc);
            st_blk<BS, true, false>(r + row0, BS, rv);
            st_blk<BS, true, false>(p + row0, BS, zv);
        } else {
            const int t = (int)(n - row0);
            ld_blk<BS, false, false>(b + row0, t, bv);
            if (Ax) ld_blk<BS, false, false>(Ax + row0, t, av);
#pragma unroll
            for (int i = 0; i < BS; ++i) rv[i] = bv[i] - (Ax ? av[i] : 0.0);
            apply_w<BS, false>(W, wld, k, t, rv, zv, acc);
            st_blk<BS, false, false>(r + row0, t, rv);
            st_blk<BS, false, false>(p + row0, t, zv);
        }
    }
    grid_sum_last_block_n<2>(acc, partials, ticket, out, 3u, stride);
}

// r -= alpha Ap (alpha = r.z_old / p.Ap); z = W r stored; out[0] = r.r,
// out[stride] = r.z from the one pass  (32 + 8 BS bytes per row)
template <int BS>
__global__ __launch_bounds__(kNT) void k_pcgb_update_r_f64(int64_t n, int64_t nblk, double *__restrict__ r,
                                                           const double *__restrict__ Ap,
                                                           const double *__restrict__ W, int64_t wld,
                                                           double *__restrict__ z, const double *rz_old,
                                                           const double *pAp, double *out, int stride, double *partials,
                                                           unsigned *ticket, const int64_t *gate) {
#pragma clang fp contract(off)
    if (gate && *gate) return;
    const double nalpha = -cg_ratio(*rz_old, *pAp);
    double acc[2] = {0.0, 0.0};
    for (int64_t k = (int64_t)blockIdx.x * kNT + threadIdx.x; k < nblk; k += (int64_t)gridDim.x * kNT) {
        const int64_t row0 = k * BS;
        double rv[BS], av[BS], zv[BS];
        if (n - row0 >= BS) {
            ld_blk<BS, true, true>(r + row0, BS, rv);
            ld_blk<BS, true, true>(Ap + row0, BS, av);
#pragma unroll
            for (int i = 0; i < BS; ++i) rv[i] = __builtin_fma(nalpha, av[i], rv[i]);
            apply_w<BS, true>(W, wld, k, BS, rv, zv, acc);
            st_blk<BS, true, true>(r + row0, BS, rv);
            st_blk<BS, true, false>(z + row0, BS, zv);
        } else {
            const int t = (int)(n - row0);
            ld_blk<BS, false, true>(r + row0, t, rv);
            ld_blk<BS, false, true>(Ap + row0, t, av);
#pragma unroll
            for (int i = 0; i < BS; ++i) rv[i] = __builtin_fma(nalpha, av[i], rv[i]);
            apply_w<BS, false>(W, wld, k, t, rv, zv, acc);
            st_blk<BS, false, true>(r + row0, t, rv);
            st_blk<BS, false, false>(z + row0, t, zv);
        }
    }
    grid_sum_last_block_n<2>(acc, partials, ticket, out, 3u, stride);
}

// x += alpha p; then, if rr != nullptr and the loop goes on, p = z + beta p with
// the stored z and beta = r.z_new / r.z_old  (40 bytes per row).  The stopping
// decision and the gate are k_pcg_update_xp_f64's, on r.r.
__global__ __launch_bounds__(kNT) void k_pcgb_update_xp_f64(int64_t n, double *__restrict__ x, double *__restrict__ p,
                                                            const double *__restrict__ z, const double *rz_old,
                                                            const double *pAp, const double *rr, const double *rz_new,
                                                            ConvArgs cv) {
#pragma clang fp contract(off)
    const StopStep st = gated_stop(cv, rr != nullptr, [&] { return rr ? *rr : 0.0; });
    if (!st.live) return;
    const bool upd_p = st.upd_p;
    const double rzo = *rz_old;
    const double alpha = cg_ratio(rzo, *pAp);
    const double beta = upd_p ? cg_ratio(*rz_new, rzo) : 0.0;
    const auto body = [&](int64_t i, auto io, auto xv, auto pv, auto zv) {
#pragma clang fp contract(off)
        io.st(x + i, vfma(alpha, pv, xv));
        if (upd_p) io.st(p + i, vfma(beta, pv, zv));
    };
    vec_pass<true, 2>(n, body, vin(x), vin(p), vopt<0>(z, upd_p));  // z: the r update's plain stores, read back plainly
}

// One-time set-up, one row per lane over the nblk * bs rows of the blocks:
// D[row * bs + j] = the sum, from +0.0 in stored order, of the row's entries
// whose column is (row / bs) * bs + j; +0.0 where there is none, and in the
// rows past n of a short last block (its columns past n match no entry: the
// indices passed cgx_csr_check).  D is block after block, row-major inside one.
// VT = float (cgx_set_precond_block on a float-valued context): each entry is
// widened exactly and the sums are the same double sums.
template <class VT>
__global__ __launch_bounds__(kNT) void k_csr_diag_blocks(int64_t n, int bs, int64_t rows,
                                                         const int64_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ col_idx,
                                                         const VT *__restrict__ values, double *__restrict__ D) {
#pragma clang fp contract(off)
    constexpr int kMaxBs = 8;
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kNT) {
        const int64_t row0 = (i / bs) * bs;
        double d[kMaxBs];
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j) d[j] = 0.0;
        if (i < n) {
            const int64_t e1 = row_ptr[i + 1];
            for (int64_t e = row_ptr[i]; e < e1; ++e) {
                const int64_t c = (int64_t)col_idx[e] - row0;
                const double v = (double)values[e];
#pragma unroll
                for (int j = 0; j < kMaxBs; ++j) d[j] = (c == j) ? d[j] + v : d[j];
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j)
            if (j < bs) D[i * bs + j] = d[j];
    }
}

inline unsigned grid_blk(int64_t nblk) { return grid_1d(nblk, kNT, 2048); }

template <int BS>
hipError_t launch_residual(int64_t n, int64_t nblk, const double *b, const double *Ax, const double *W, int64_t wld,
                           double *r, double *p, double *out, int stride, const RedWs &ws, hipStream_t s,
                           int64_t *clear2) {
    hipLaunchKernelGGL(k_pcgb_residual_f64<BS>, dim3(grid_blk(nblk)), dim3(kNT), 0, s, n, nblk, b, Ax, W, wld, r, p, out,
                       stride, ws.partials, ws.tickets + T_RESID, clear2);
    return hipGetLastError();
}

template <int BS>
hipError_t launch_update_r(int64_t n, int64_t nblk, double *r, const double *Ap, const double *W, int64_t wld, double *z,
                           const double *rz_old, const double *pAp, double *out, int stride, const RedWs &ws,
                           hipStream_t s, const int64_t *gate) {
    hipLaunchKernelGGL(k_pcgb_update_r_f64<BS>, dim3(grid_blk(nblk)), dim3(kNT), 0, s, n, nblk, r, Ap, W, wld, z, rz_old,
                       pAp, out, stride, ws.partials, ws.tickets + T_XR, gate);
    return hipGetLastError();
}

}  // namespace

hipError_t pcgb_residual_f64(int bs, int64_t n, const double *b, const double *Ax, const double *W, int64_t wld,
                             double *r, double *p, double *out, int stride, const RedWs &ws, hipStream_t s,
                             int64_t *clear2) {
    if (bs < 2 || bs > kMaxPcBlock || n < 1) return hipErrorInvalidValue;
    const int64_t nblk = (n + bs - 1) / bs;
    if (wld < nblk || !(al16(b) && al16(Ax) && al16(r) && al16(p))) return hipErrorInvalidValue;
#define CGX_CALL_(BS) launch_residual<BS>(n, nblk, b, Ax, W, wld, r, p, out, stride, ws, s, clear2)
    switch (bs) {
        case 2: return CGX_CALL_(2);
        case 3: return CGX_CALL_(3);
        case 4: return CGX_CALL_(4);
        case 5: return CGX_CALL_(5);
        case 6: return CGX_CALL_(6);
        case 7: return CGX_CALL_(7);
        default: return CGX_CALL_(8);
    }
#undef CGX_CALL_
}

hipError_t pcgb_update_r_f64(int bs, int64_t n, double *r, const double *Ap, const double *W, int64_t wld, double *z,
                             const double *rz_old, const double *pAp, double *out, int stride, const RedWs &ws,
                             hipStream_t s, const int64_t *gate) {
    if (bs < 2 || bs > kMaxPcBlock || n < 1) return hipErrorInvalidValue;
    const int64_t nblk = (n + bs - 1) / bs;
    if (wld < nblk || !(al16(r) && al16(Ap) && al16(z))) return hipErrorInvalidValue;
#define CGX_CALL_(BS) launch_update_r<BS>(n, nblk, r, Ap, W, wld, z, rz_old, pAp, out, stride, ws, s, gate)
    switch (bs) {
        case 2: return CGX_CALL_(2);
        case 3: return CGX_CALL_(3);
        case 4: return CGX_CALL_(4);
        case 5: return CGX_CALL_(5);
        case 6: return CGX_CALL_(6);
        case 7: return CGX_CALL_(7);
        default: return CGX_CALL_(8);
    }
#undef CGX_CALL_
}

hipError_t pcgb_update_xp_f64(int64_t n, double *x, double *p, const double *z, const double *rz_old,
                              const double *pAp, const double *rr, const double *rz_new, hipStream_t s, double eps,
                              int64_t k, int64_t *kdone, double *rrfinal, int64_t *hrec) {
    if (!(al16(x) && al16(p) && al16(z))) return hipErrorInvalidValue;
    const ConvArgs cv = conv_args(eps, k, kdone, rrfinal, hrec);
    hipLaunchKernelGGL(k_pcgb_update_xp_f64, dim3(grid_vec(n)), dim3(kNT), 0, s, n, x, p, z, rz_old, pAp, rr, rz_new,
                       cv);
    return hipGetLastError();
}

hipError_t csr_diag_blocks_f64(int64_t n, int bs, const int64_t *row_ptr, const int32_t *col_idx,
                               CsrValues values, double *D, hipStream_t s) {
    if (bs < 2 || bs > kMaxPcBlock || n < 1) return hipErrorInvalidValue;
    const int64_t rows = (n + bs - 1) / bs * bs;
    if (values.f32)
        hipLaunchKernelGGL(k_csr_diag_blocks<float>, dim3(grid_1d(rows, kNT, 65536)), dim3(kNT), 0, s, n, bs, rows,
                           row_ptr, col_idx, static_cast<const float *>(values.p), D);
    else
        hipLaunchKernelGGL(k_csr_diag_blocks<double>, dim3(grid_1d(rows, kNT, 65536)), dim3(kNT), 0, s, n, bs, rows,
                           row_ptr, col_idx, static_cast<const double *>(values.p), D);
    return hipGetLastError();
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_pcg_block() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_csr_diag_blocks<double>));
}

}  // namespace cgx
