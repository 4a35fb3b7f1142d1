// cgx_spmm.hip -- the sparse matVec of a cgx_create_csr_nrhs context: one pass
// over a CSR matrix (row_ptr int64[n+1], col_idx int32[nnz], values
// double[nnz] or, on a float-valued context, float[nnz]) multiplied by K vectors, Out_j = A V_j for j < nrhs, fp64.
//
// The CSR-vector form of k_spmv_csr_f64 (cgx_spmv.hip): T consecutive lanes own
// one row, a wave covers 64/T consecutive rows, waves walk the row groups with
// a grid-stride.  values[e] and col_idx[e] are loaded once per entry (load_a:
// default policy or non-temporal) and multiplied by the K gathered elements
// V[j*ldv + col_idx[e]], 8-byte default-policy loads (an odd ldv or an
// unaligned V needs no path of its own).  K = nrhs_width(nrhs) is 2, 4 or 8;
// columns nrhs..K-1 read column 0 again and are never stored, as in
// k_matvec_nrhs_f64.
//
// Layout of the K vectors: column after column (column j at V + j*ldv, Out:
// ldo, pown: ldp), the layout the K-column vector kernels of
// cgx_matvec_nrhs.hip work on.  (An interleaved n x K layout would make the K
// gathers of an entry one contiguous read; it needs update kernels of its own
// and is not built)
//
// Summation order per column (a contract): exactly k_spmv_csr_f64's at the
// same T -- sub-lane l starts from +0.0 and adds entries s+l, s+l+T, ... in
// stored order with one FMA each; the T partial sums are combined as
// v[l] += v[l ^ o] for o = T/2, ..., 1.  Column j is therefore cgx_spmv_csr's
// result on column j bit for bit at the same T, whatever K, the load policy,
// the grid, or the trips a sub-lane keeps in flight.  Float-stored values
// (VT = float) are widened with (double) before the same FMAs, as in
// k_spmv_csr_f64: the double kernel's bits on (double)values[e].
//
// The kernel does not range-check col_idx: every host path checks the
// structure first (cgx_csr_check).
#include "cgx_matvec_core.h"

#include <algorithm>

namespace cgx {
namespace {

// Trips a sub-lane has in flight (kSpmvU's counterpart): a trip holds one value,
// one index and K gathered elements, 3 + 2 K registers.  The FMAs of a column
// run in trip order whatever this is.  Measured as whole sweeps (best plan, ms
// per launch, banded / Poisson; profiles/spmm_ab_variants.jsonl):
// K = 4 with two trips 0.364 / 0.834, with four 0.321 / 0.676; K = 8 with four
// trips (132 VGPRs, 3 waves per SIMD) 0.478 / 1.325, with two 0.503 / 1.161.
template <int K>
constexpr int kSpmmU = K == 8 ? 2 : 4;

template <class VT, int T, int K, int NT>
__global__ __launch_bounds__(kNT) void k_spmm_csr_f64(const int64_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ col_idx,
                                                       const VT *__restrict__ values, int64_t rows, int nrhs,
                                                       const double *__restrict__ V, int64_t ldv,
                                                       double *__restrict__ Out, int64_t ldo,
                                                       const double *__restrict__ pown, int64_t ldp, double *dot_out,
                                                       double *partials, unsigned *ticket, const int64_t *gate,
                                                       int64_t *ts) {
    if (gate && *gate) return;  // every column stopped in an earlier iteration (device-side gating)
    ts_start(ts);
    constexpr int RW = 64 / T;  // rows per wave
    constexpr int U = kSpmmU<K>;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int sub = lane & (T - 1), rloc = lane / T;
    const int64_t ngroups = (rows + RW - 1) / RW;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    const double *vj[K];
#pragma unroll
    for (int j = 0; j < K; ++j) vj[j] = V + (j < nrhs ? j : 0) * ldv;
    double dacc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) dacc[j] = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t i = g * RW + rloc;
        const bool live = i < rows;  // rows past the end: no loads, no store
        int64_t s = 0, e = 0;
        if (live) {
            s = row_ptr[i];
            e = row_ptr[i + 1];
        }
        double acc[K];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = 0.0;
        for (int64_t k = s + sub; k < e; k += (int64_t)U * T) {
            VT a[U];
            double x[U][K];
            int32_t c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = k + (int64_t)u * T < e;
                a[u] = ok ? load_a<NT>(values + k + (int64_t)u * T) : VT(0);
                c[u] = ok ? load_a<NT>(col_idx + k + (int64_t)u * T) : -1;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < K; ++j) x[u][j] = c[u] >= 0 ? vj[j][c[u]] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0) {
#pragma unroll
                    for (int j = 0; j < K; ++j) acc[j] = __builtin_fma((double)a[u], x[u][j], acc[j]);
                }
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int o = T / 2; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
        if (live && sub == 0) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < nrhs) store_row(i, acc[j], Out + j * ldo, pown ? pown + j * ldp : nullptr, dacc[j]);
        }
    }
    if (pown) grid_sum_last_block_n<K>(dacc, partials, ticket, dot_out, (1u << nrhs) - 1u);
    ts_end(ts);
}

template <class VT>
using SpmmFn = decltype(&k_spmm_csr_f64<VT, 8, 2, 1>);

template <class VT, int K, int NT>
SpmmFn<VT> pick_spmm_t(int T) {
    switch (T) {
        case 2: return k_spmm_csr_f64<VT, 2, K, NT>;
        case 4: return k_spmm_csr_f64<VT, 4, K, NT>;
        case 8: return k_spmm_csr_f64<VT, 8, K, NT>;
        case 16: return k_spmm_csr_f64<VT, 16, K, NT>;
        case 32: return k_spmm_csr_f64<VT, 32, K, NT>;
        case 64: return k_spmm_csr_f64<VT, 64, K, NT>;
        default: return nullptr;
    }
}
template <class VT, int NT>
SpmmFn<VT> pick_spmm_nt(int K, int T) {
    return K == 2   ? pick_spmm_t<VT, 2, NT>(T)
           : K == 4 ? pick_spmm_t<VT, 4, NT>(T)
           : K == 8 ? pick_spmm_t<VT, 8, NT>(T)
                    : nullptr;
}
// the instantiated plan's kernel, or nullptr: K vectors, T lanes per row, load policy 2 or 8;
// the same (K, T, policy) list for double (VT = double) and float values
template <class VT>
SpmmFn<VT> pick_spmm(int K, int T, int nt) {
    return nt == 8 ? pick_spmm_nt<VT, 1>(K, T) : nt == 2 ? pick_spmm_nt<VT, 0>(K, T) : nullptr;
}
const void *spmm_fn(int K, int T, int nt, bool f32) {
    return f32 ? reinterpret_cast<const void *>(pick_spmm<float>(K, T, nt))
               : reinterpret_cast<const void *>(pick_spmm<double>(K, T, nt));
}

template <class VT>
hipError_t launch_spmm(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, const void *values,
                       int64_t rows, int nrhs, const double *V, int64_t ldv, double *Out, int64_t ldo,
                       const double *pown, int64_t ldp, double *dot_out, const RedWs &ws, hipStream_t s,
                       const int64_t *gate, int64_t *ts) {
    hipLaunchKernelGGL(pick_spmm<VT>(pl.nrhs, 64 / pl.R, pl.nt), dim3(pl.blocks), dim3(kNT), 0, s, row_ptr, col_idx,
                       static_cast<const VT *>(values), rows, nrhs, V, ldv, Out, ldo, pown, ldp, dot_out, ws.partials,
                       ws.tickets + TN_MATVEC, gate, ts);
    return hipGetLastError();
}

}  // namespace

bool spmm_csr_plan_ok(int K, int T, int nt) { return pick_spmm<double>(K, T, nt) != nullptr; }

MatvecPlan plan_spmm_csr(int device, int64_t rows, int64_t nnz, int K, int T, int nt, int blocks_per_cu, bool f32) {
    MatvecPlan pl;
    pl.csr = 1;
    pl.nrhs = K;
    pl.U = 1;
    // Measured on MI355X, every (T, policy) of a width interleaved in five
    // rounds in one process with the one-system context's default plan
    // (tools/spmm_ab.py, profiles/spmm_ab_*.jsonl; ms per launch, round-to-round
    // spread below 1 %), T = 2 / 4 / 8 / 16 / 32 / 64 with policy 2:
    //   5-point Poisson, m = 4096 (mean row length 5; one system 0.345 at T = 2):
    //     K = 2: 0.467 / 0.520 / 0.827 / 1.501 / 2.895 / 5.780
    //     K = 4: 0.650 / 0.965 / 1.648 / 3.095 / 5.946 / 11.97
    //     K = 8: 1.171 / 1.615 / 2.529 / 4.648 / 9.150 / 19.25
    //   banded, n = 2^20, 65 entries per full row (one system 0.203 at T = 16):
    //     K = 2: 0.466 / 0.288 / 0.249 / 0.259 / 0.316 / 0.451
    //     K = 4: 0.511 / 0.344 / 0.320 / 0.374 / 0.505 / 0.888
    //     K = 8: 0.706 / 0.511 / 0.513 / 0.601 / 0.844 / 1.371
    // Policy 8 is slower at every T, K and matrix (best: 0.515 / 0.678 / 1.209
    // and 0.302 / 0.394 / 0.599): policy 2 at every size.  plan_spmv_csr's
    // rule (T <= mean / 4) would take T = 16 on the banded matrix, 4-17 %
    // behind T = 8 at every K: with K gathers per entry the best T is half the
    // SpMV's there, and still 2 at mean 5.  So T = the largest instantiated
    // T <= mean / 8, at least 2, for every K (at K = 8 on the banded matrix
    // T = 4 and T = 8 tie).  Means other than 5 and 65 and skewed row lengths
    // are not measured.
    // nnz < 0 (the kernel-level call, which does not know it): T = 8.
    int t = 8;
    if (nnz >= 0 && rows > 0) {
        const int64_t mean = nnz / rows;
        for (t = 2; t < 64 && 2 * t <= mean / 8;) t *= 2;
    }
    pl.R = 64 / t;
    pl.nt = 2;
    // CGX_SPMM_PLAN="T=..,nt=..,bpc=..": taken when it names an instantiated plan, then the arguments
    const int eT = env_opt("CGX_SPMM_PLAN", "T", t), en = env_opt("CGX_SPMM_PLAN", "nt", pl.nt);
    if (spmm_csr_plan_ok(K, eT, en)) pl.R = 64 / eT, pl.nt = en;
    if (T > 0) pl.R = spmm_csr_plan_ok(K, T, 8) ? 64 / T : 0;
    if (nt >= 0) pl.nt = nt;
    if (pl.R < 1 || !spmm_csr_plan_ok(K, 64 / pl.R, pl.nt)) pl.R = 64 / t, pl.nt = 2;
    pl.blocks = plan_grid(spmm_fn(K, 64 / pl.R, pl.nt, f32), device, rows, pl.R, 8, "CGX_SPMM_PLAN", blocks_per_cu);
    return pl;
}

hipError_t spmm_csr_f64(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, int nrhs, const double *V, int64_t ldv, double *Out, int64_t ldo,
                        const double *pown, int64_t ldp, double *dot_out, const RedWs &ws, hipStream_t s,
                        const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    if (nrhs < 1 || nrhs > kMaxNrhs || !pl.csr || pl.nrhs != nrhs_width(nrhs) || pl.R < 1 || pl.R > 32 ||
        !spmm_csr_plan_ok(pl.nrhs, 64 / pl.R, pl.nt) || pl.blocks < 1 || pl.blocks > kMaxRedBlocks)
        return hipErrorInvalidValue;
    return values.f32 ? launch_spmm<float>(pl, row_ptr, col_idx, values.p, rows, nrhs, V, ldv, Out, ldo, pown, ldp,
                                           dot_out, ws, s, gate, ts)
                      : launch_spmm<double>(pl, row_ptr, col_idx, values.p, rows, nrhs, V, ldv, Out, ldo, pown, ldp,
                                            dot_out, ws, s, gate, ts);
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_spmm() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_spmm_csr_f64<double, 8, 2, 1>));
}

}  // namespace cgx
