// cgx_csr_core.h -- internal to libcgx, for its two sparse kernel files: the one
// sparse matVec kernel k_csr_mult_f64, its pick table, launch and plan rule, all
// with internal linkage (each file gets the widths it names).  cgx_spmv.hip
// instantiates it at width K = 1 (the SpMV of a cgx_create_csr context),
// cgx_spmm.hip at K = 2, 4, 8 (the SpMM of a cgx_create_csr_nrhs context): two
// code objects, so a one-system context loads 24 kernels, not 96.  The body
// stays inside the __global__ template: moved into a __device__ function that
// both files' kernels called, every K = 8 instantiation took 107-111 VGPRs in
// place of 91-95 (4 waves per SIMD in place of 5) and every K = 4 float one 4-5
// more (make asm), the effect cgx_matvec_core.h records for the dense kernels.
//
// One pass over a CSR matrix (row_ptr int64[n+1], col_idx int32[nnz], values
// double[nnz] or, on a float-valued context, float[nnz]) multiplied by K
// vectors, Out_j = A V_j for j < nrhs, fp64.
//
// CSR-vector form.  T consecutive lanes own one row (T = 2 .. 64), so a wave
// covers 64/T consecutive rows and its loads of values and col_idx are
// contiguous across those rows: sub-lane l of row i reads entries s+l, s+l+T,
// ... of [s, e) = [row_ptr[i], row_ptr[i+1]).  Waves walk the groups of 64/T
// rows with a grid-stride, as for_row_groups does (cgx_matvec_core.h).  The two
// streamed arrays are read once per entry (load_a: default policy or
// non-temporal); the gathers V[j*ldv + col_idx[e]] are the only data reused and
// take 8-byte default-policy loads (an odd ldv or an unaligned V needs no path
// of its own).  K = 1 is called with nrhs = 1 and strides 0; otherwise
// K = nrhs_width(nrhs), and columns nrhs..K-1 read column 0 again and are never
// stored, as in k_matvec_nrhs_f64.
//
// Layout of the K vectors: column after column (column j at V + j*ldv, Out:
// ldo, pown: ldp), the layout the K-column vector kernels of
// cgx_matvec_nrhs.hip work on.  (An interleaved n x K layout would make the K
// gathers of an entry one contiguous read; it needs update kernels of its own
// and is not built)
//
// Summation order per column (a contract; tests/_spmv_order.py states it on the
// CPU): sub-lane l starts from +0.0 and adds its entries in stored order with
// one FMA each; the T partial sums are combined as wave_sum combines 64,
// v[l] += v[l ^ o] for o = T/2, ..., 1.  Columns need not be sorted and a
// duplicate column is two terms.  A row's sum depends on T only: not on K, the
// load policy, the grid, the trips a sub-lane keeps in flight, or where the row
// falls in a wave.  Column j of an SpMM is therefore the SpMV's result on
// column j bit for bit at the same T: they are one body.
//
// Float-stored values (VT = float, cgx_set_csr_f32): an entry is loaded as 4
// bytes through the same policy and widened with (double), which is exact,
// denormals included; the FMA, its order and everything after it are the double
// kernel's.  So the row sum is the double kernel's on (double)values[e] bit for
// bit, and an entry streams 8 bytes in place of 12.
//
// The fused dots pown_j . Out_j go through grid_sum_last_block_n<K>, which sums
// a column exactly as grid_sum_last_block sums its one value (cgx_device.h).
//
// No load balancing: a row of length L costs ceil(L / T) trips
// of its T lanes while the wave's other rows wait.
//
// The kernel does not range-check col_idx: every host path checks the
// structure first (cgx_csr_check).
#pragma once
#include "cgx_matvec_core.h"

namespace cgx {
namespace {

// Trips a sub-lane has in flight: the loads of U trips (values and col_idx,
// then the gathers) are issued before their FMAs, which run in trip order.  A
// trip past the row's end loads nothing and adds nothing.  A trip holds one
// value, one index and K gathered elements, 3 + 2 K registers.  The FMAs of a
// column run in trip order whatever this is.  Measured as whole sweeps (best plan, ms
// per launch, banded / Poisson; profiles/spmm_ab_variants.jsonl):
// K = 4 with two trips 0.364 / 0.834, with four 0.321 / 0.676; K = 8 with four
// trips (132 VGPRs, 3 waves per SIMD) 0.478 / 1.325, with two 0.503 / 1.161.
template <int K>
constexpr int kSpmmU = K == 8 ? 2 : 4;

// the one-system and the nrhs reduction scratch index the same ticket
static_assert((int)T_MATVEC == (int)TN_MATVEC, "k_csr_mult_f64 takes one matVec ticket for every width");

template <class VT, int T, int K, int NT>
__global__ __launch_bounds__(kNT) void k_csr_mult_f64(const int64_t *__restrict__ row_ptr,
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
using CsrFn = decltype(&k_csr_mult_f64<VT, 8, 1, 1>);  // the same type at every (T, K, policy)

template <class VT, int K, int NT>
CsrFn<VT> pick_csr_t(int T) {
    switch (T) {
        case 2: return k_csr_mult_f64<VT, 2, K, NT>;
        case 4: return k_csr_mult_f64<VT, 4, K, NT>;
        case 8: return k_csr_mult_f64<VT, 8, K, NT>;
        case 16: return k_csr_mult_f64<VT, 16, K, NT>;
        case 32: return k_csr_mult_f64<VT, 32, K, NT>;
        case 64: return k_csr_mult_f64<VT, 64, K, NT>;
        default: return nullptr;
    }
}
template <class VT, int NT, int... Ks>
CsrFn<VT> pick_csr_nt(int K, int T) {
    CsrFn<VT> fn = nullptr;
    ((K == Ks ? void(fn = pick_csr_t<VT, Ks, NT>(T)) : void()), ...);
    return fn;
}
// The instantiated plan's kernel, or nullptr: K vectors, T lanes per row, load
// policy 2 or 8; the same (K, T, policy) list for double (VT = double) and
// float values.  Ks... are the widths the including file instantiates (1, or
// 2, 4, 8): naming a kernel here is what puts it into that file's code object.
template <class VT, int... Ks>
CsrFn<VT> pick_csr(int K, int T, int nt) {
    return nt == 8 ? pick_csr_nt<VT, 1, Ks...>(K, T) : nt == 2 ? pick_csr_nt<VT, 0, Ks...>(K, T) : nullptr;
}
template <int... Ks>
bool csr_plan_ok(int K, int T, int nt) {
    return pick_csr<double, Ks...>(K, T, nt) != nullptr;
}

template <class VT, int... Ks>
hipError_t launch_csr(const MatvecPlan &pl, int K, const int64_t *row_ptr, const int32_t *col_idx, const void *values,
                      int64_t rows, int nrhs, const double *V, int64_t ldv, double *Out, int64_t ldo,
                      const double *pown, int64_t ldp, double *dot_out, const RedWs &ws, hipStream_t s,
                      const int64_t *gate, int64_t *ts) {
    hipLaunchKernelGGL((pick_csr<VT, Ks...>(K, 64 / pl.R, pl.nt)), dim3(pl.blocks), dim3(kNT), 0, s, row_ptr, col_idx,
                       static_cast<const VT *>(values), rows, nrhs, V, ldv, Out, ldo, pown, ldp, dot_out, ws.partials,
                       ws.tickets + T_MATVEC, gate, ts);
    return hipGetLastError();
}
// Out_j = A V_j under a plan of width K: what both files' entry points check
// of the plan, then the launch for the value type.
template <int... Ks>
hipError_t csr_mult_f64(const MatvecPlan &pl, int K, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, int nrhs, const double *V, int64_t ldv, double *Out, int64_t ldo,
                        const double *pown, int64_t ldp, double *dot_out, const RedWs &ws, hipStream_t s,
                        const int64_t *gate, int64_t *ts) {
    if (!pl.csr || pl.R < 1 || pl.R > 32 || !csr_plan_ok<Ks...>(K, 64 / pl.R, pl.nt) || pl.blocks < 1 ||
        pl.blocks > kMaxRedBlocks)
        return hipErrorInvalidValue;
    return values.f32 ? launch_csr<float, Ks...>(pl, K, row_ptr, col_idx, values.p, rows, nrhs, V, ldv, Out, ldo, pown,
                                                 ldp, dot_out, ws, s, gate, ts)
                      : launch_csr<double, Ks...>(pl, K, row_ptr, col_idx, values.p, rows, nrhs, V, ldv, Out, ldo, pown,
                                                  ldp, dot_out, ws, s, gate, ts);
}

// The plan of width K: T <= 0 / nt < 0 / blocks_per_cu <= 0 pick the defaults.
template <int... Ks>
MatvecPlan plan_csr(int device, int64_t rows, int64_t nnz, int K, int T, int nt, int blocks_per_cu, bool f32) {
    MatvecPlan pl;
    pl.csr = 1;
    pl.nrhs = K == 1 ? 0 : K;
    pl.U = 1;
    // K = 1.  Measured on MI355X, every (T, policy) interleaved in five rounds in one
    // process (tools/spmv_ab.py, profiles/spmv_ab_*.jsonl; ms per launch,
    // round-to-round spread below 0.5 %):
    //   5-point Poisson, m = 4096 (16.8 M rows, mean row length 5, 1.41 GB):
    //     T = 2 / 4 / 8 / 16 / 32 / 64 with policy 2: 0.330 / 0.365 / 0.600 /
    //     1.104 / 2.120 / 4.204; with policy 8: 0.391 / 0.369 / 0.606 / 1.132 /
    //     2.230 / 4.484
    //   banded, n = 2^20, 65 entries per full row (0.84 GB):
    //     policy 2: 0.446 / 0.263 / 0.216 / 0.204 / 0.239 / 0.349; policy 8:
    //     0.765 / 0.445 / 0.311 / 0.242 / 0.240 / 0.356
    // The best T is the one that gives a sub-lane about kSpmmU<1> = 4 entries (2 at
    // mean 5, 16 at mean 65): more rows per wave keep more of its lanes loading,
    // and the starting rule "T >= the mean row length" with policy 8 (T = 8 and
    // 64 here) ran at 0.56x of the best plan on both (spmv_ab_*_startrule.jsonl).  So T = the largest instantiated T <=
    // mean / 4, at least 2.  Means other than 5 and 65 are not measured; skewed
    // row lengths are not measured (no load balancing).
    // Default-policy loads beat non-temporal ones at every T on both matrices,
    // both far above the 64 MiB below which plan_matvec_f64 keeps policy 2 for
    // the MALL: policy 2 at every size (sizes below 0.8 GB not measured).
    //
    // K >= 2.  Measured on MI355X, every (T, policy) of a width interleaved in five
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
    // and 0.302 / 0.394 / 0.599): policy 2 at every size.  The K = 1
    // rule (T <= mean / 4) would take T = 16 on the banded matrix, 4-17 %
    // behind T = 8 at every K: with K gathers per entry the best T is half the
    // SpMV's there, and still 2 at mean 5.  So T = the largest instantiated
    // T <= mean / 8, at least 2, for every K >= 2 (at K = 8 on the banded matrix
    // T = 4 and T = 8 tie).  Means other than 5 and 65 and skewed row lengths
    // are not measured.
    // nnz < 0 (the kernel-level call, which does not know it): T = 8.
    int t = 8;
    if (nnz >= 0 && rows > 0) {
        const int64_t mean = nnz / rows;
        for (t = 2; t < 64 && 2 * t <= mean / (K == 1 ? 4 : 8);) t *= 2;
    }
    pl.R = 64 / t;
    pl.nt = 2;
    // CGX_SPMV_PLAN (K = 1) or CGX_SPMM_PLAN = "T=..,nt=..,bpc=..": taken when it names an instantiated
    // plan (as plan_listed takes the dense families' overrides), then the arguments
    const char *env = K == 1 ? "CGX_SPMV_PLAN" : "CGX_SPMM_PLAN";
    const int eT = env_opt(env, "T", t), en = env_opt(env, "nt", pl.nt);
    if (csr_plan_ok<Ks...>(K, eT, en)) pl.R = 64 / eT, pl.nt = en;
    if (T > 0) pl.R = csr_plan_ok<Ks...>(K, T, 8) ? 64 / T : 0;
    if (nt >= 0) pl.nt = nt;
    if (pl.R < 1 || !csr_plan_ok<Ks...>(K, 64 / pl.R, pl.nt)) pl.R = 64 / t, pl.nt = 2;
    const void *fn = f32 ? reinterpret_cast<const void *>(pick_csr<float, Ks...>(K, 64 / pl.R, pl.nt))
                         : reinterpret_cast<const void *>(pick_csr<double, Ks...>(K, 64 / pl.R, pl.nt));
    pl.blocks = plan_grid(fn, device, rows, pl.R, 8, env, blocks_per_cu);
    return pl;
}

}  // namespace
}  // namespace cgx
