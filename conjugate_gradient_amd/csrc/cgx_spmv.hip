// cgx_spmv.hip -- the sparse matVec of a cgx_create_csr context: A in CSR
// storage (row_ptr int64[n+1], col_idx int32[nnz], values double[nnz] or, on a
// float-valued context, float[nnz]), fp64.
//
// CSR-vector form.  T consecutive lanes own one row (T = 2 .. 64), so a wave
// covers 64/T consecutive rows and its loads of values and col_idx are
// contiguous across those rows: sub-lane l of row i reads entries s+l, s+l+T,
// ... of [s, e) = [row_ptr[i], row_ptr[i+1]).  Waves walk the groups of 64/T
// rows with a grid-stride, as for_row_groups does (cgx_matvec_core.h).  The two
// streamed arrays are read once (load_a: default policy or non-temporal); the
// gather v[col_idx[e]] is the only data reused and takes default-policy loads.
//
// Summation order (a contract; tests/_spmv_order.py states it on the CPU):
// sub-lane l starts from +0.0 and adds its entries in stored order with one
// FMA each; the T partial sums are combined as wave_sum combines 64,
// v[l] += v[l ^ o] for o = T/2, ..., 1.  Columns need not be sorted and a
// duplicate column is two terms.  A row's sum depends on T only: not on the
// load policy, the grid, or where the row falls in a wave.
//
// Float-stored values (VT = float, cgx_set_csr_f32): an entry is loaded as 4
// bytes through the same policy and widened with (double), which is exact,
// denormals included; the FMA, its order and everything after it are the double
// kernel's.  So the row sum is the double kernel's on (double)values[e] bit for
// bit, and an entry streams 8 bytes in place of 12.
//
// No load balancing: a row of length L costs ceil(L / T) trips
// of its T lanes while the wave's other rows wait.
//
// The kernel does not range-check col_idx: every host path checks the
// structure first (cgx_csr_check).
#include "cgx_matvec_core.h"

#include <algorithm>

namespace cgx {
namespace {

// Entries a sub-lane has in flight: the loads of kSpmvU trips (values and
// col_idx, then the gathers) are issued before their FMAs, which run in trip
// order.  A trip past the row's end loads nothing and adds nothing.
constexpr int kSpmvU = 4;

template <class VT, int T, int NT>
__global__ __launch_bounds__(kNT) void k_spmv_csr_f64(const int64_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ col_idx,
                                                       const VT *__restrict__ values, int64_t rows,
                                                       const double *__restrict__ v, double *__restrict__ out,
                                                       const double *__restrict__ pown, double *dot_out,
                                                       double *partials, unsigned *ticket, const int64_t *gate,
                                                       int64_t *ts) {
    if (gate && *gate) return;  // the solve converged in an earlier iteration (device-side gating)
    ts_start(ts);
    constexpr int RW = 64 / T;  // rows per wave
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int sub = lane & (T - 1), rloc = lane / T;
    const int64_t ngroups = (rows + RW - 1) / RW;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    double dacc = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t i = g * RW + rloc;
        const bool live = i < rows;  // rows past the end: no loads, no store
        int64_t s = 0, e = 0;
        if (live) {
            s = row_ptr[i];
            e = row_ptr[i + 1];
        }
        double acc = 0.0;
        for (int64_t k = s + sub; k < e; k += (int64_t)kSpmvU * T) {
            VT a[kSpmvU];
            double x[kSpmvU];
            int32_t c[kSpmvU];
#pragma unroll
            for (int u = 0; u < kSpmvU; ++u) {
                const bool ok = k + (int64_t)u * T < e;
                a[u] = ok ? load_a<NT>(values + k + (int64_t)u * T) : VT(0);
                c[u] = ok ? load_a<NT>(col_idx + k + (int64_t)u * T) : -1;
            }
#pragma unroll
            for (int u = 0; u < kSpmvU; ++u) x[u] = c[u] >= 0 ? v[c[u]] : 0.0;
#pragma unroll
            for (int u = 0; u < kSpmvU; ++u)
                if (c[u] >= 0) acc = __builtin_fma((double)a[u], x[u], acc);
        }
#pragma unroll
        for (int o = T / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (live && sub == 0) store_row(i, acc, out, pown, dacc);
    }
    if (pown) grid_sum_last_block(dacc, partials, ticket, dot_out);
    ts_end(ts);
}

template <class VT>
using SpmvFn = decltype(&k_spmv_csr_f64<VT, 8, 1>);

template <class VT, int NT>
SpmvFn<VT> pick_spmv_nt(int T) {
    switch (T) {
        case 2: return k_spmv_csr_f64<VT, 2, NT>;
        case 4: return k_spmv_csr_f64<VT, 4, NT>;
        case 8: return k_spmv_csr_f64<VT, 8, NT>;
        case 16: return k_spmv_csr_f64<VT, 16, NT>;
        case 32: return k_spmv_csr_f64<VT, 32, NT>;
        case 64: return k_spmv_csr_f64<VT, 64, NT>;
        default: return nullptr;
    }
}
// the instantiated plan's kernel, or nullptr: T lanes per row, load policy 2 or 8;
// the same (T, policy) list for double (VT = double) and float values
template <class VT>
SpmvFn<VT> pick_spmv(int T, int nt) {
    return nt == 8 ? pick_spmv_nt<VT, 1>(T) : nt == 2 ? pick_spmv_nt<VT, 0>(T) : nullptr;
}
const void *spmv_fn(int T, int nt, bool f32) {
    return f32 ? reinterpret_cast<const void *>(pick_spmv<float>(T, nt))
               : reinterpret_cast<const void *>(pick_spmv<double>(T, nt));
}

template <class VT>
hipError_t launch_spmv(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, const void *values,
                       int64_t rows, const double *v, double *out, const double *pown, double *dot_out,
                       const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    hipLaunchKernelGGL(pick_spmv<VT>(64 / pl.R, pl.nt), dim3(pl.blocks), dim3(kNT), 0, s, row_ptr, col_idx,
                       static_cast<const VT *>(values), rows, v, out, pown, dot_out, ws.partials,
                       ws.tickets + T_MATVEC, gate, ts);
    return hipGetLastError();
}

}  // namespace

bool spmv_csr_plan_ok(int T, int nt) { return pick_spmv<double>(T, nt) != nullptr; }

MatvecPlan plan_spmv_csr(int device, int64_t rows, int64_t nnz, int T, int nt, int blocks_per_cu, bool f32) {
    MatvecPlan pl;
    pl.csr = 1;
    pl.U = 1;
    // Measured on MI355X, every (T, policy) interleaved in five rounds in one
    // process (tools/spmv_ab.py, profiles/spmv_ab_*.jsonl; ms per launch,
    // round-to-round spread below 0.5 %):
    //   5-point Poisson, m = 4096 (16.8 M rows, mean row length 5, 1.41 GB):
    //     T = 2 / 4 / 8 / 16 / 32 / 64 with policy 2: 0.330 / 0.365 / 0.600 /
    //     1.104 / 2.120 / 4.204; with policy 8: 0.391 / 0.369 / 0.606 / 1.132 /
    //     2.230 / 4.484
    //   banded, n = 2^20, 65 entries per full row (0.84 GB):
    //     policy 2: 0.446 / 0.263 / 0.216 / 0.204 / 0.239 / 0.349; policy 8:
    //     0.765 / 0.445 / 0.311 / 0.242 / 0.240 / 0.356
    // The best T is the one that gives a sub-lane about kSpmvU = 4 entries (2 at
    // mean 5, 16 at mean 65): more rows per wave keep more of its lanes loading,
    // and the starting rule "T >= the mean row length" with policy 8 (T = 8 and
    // 64 here) ran at 0.56x of the best plan on both (spmv_ab_*_startrule.jsonl).  So T = the largest instantiated T <=
    // mean / 4, at least 2.  Means other than 5 and 65 are not measured; skewed
    // row lengths are not measured (no load balancing).
    // Default-policy loads beat non-temporal ones at every T on both matrices,
    // both far above the 64 MiB below which plan_matvec_f64 keeps policy 2 for
    // the MALL: policy 2 at every size (sizes below 0.8 GB not measured).
    // nnz < 0 (the kernel-level call, which does not know it): T = 8.
    const int64_t mean = (nnz >= 0 && rows > 0) ? nnz / rows : 32;
    int t = 2;
    while (t < 64 && 2 * t <= mean / 4) t *= 2;
    pl.R = 64 / t;
    pl.nt = 2;
    // CGX_SPMV_PLAN="T=..,nt=..,bpc=..": taken when it names an instantiated
    // plan (as plan_listed takes the dense families' overrides), then the arguments
    const int eT = env_opt("CGX_SPMV_PLAN", "T", t), en = env_opt("CGX_SPMV_PLAN", "nt", pl.nt);
    if (spmv_csr_plan_ok(eT, en)) pl.R = 64 / eT, pl.nt = en;
    if (T > 0) pl.R = spmv_csr_plan_ok(T, 8) ? 64 / T : 0;
    if (nt >= 0) pl.nt = nt;
    if (pl.R < 1 || !spmv_csr_plan_ok(64 / pl.R, pl.nt)) pl.R = 64 / t, pl.nt = 2;
    pl.blocks = plan_grid(spmv_fn(64 / pl.R, pl.nt, f32), device, rows, pl.R, 8, "CGX_SPMV_PLAN", blocks_per_cu);
    return pl;
}

hipError_t spmv_csr_f64(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, const double *v, double *out, const double *pown, double *dot_out,
                        const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    if (!pl.csr || pl.R < 1 || pl.R > 32 || !spmv_csr_plan_ok(64 / pl.R, pl.nt) || pl.blocks < 1)
        return hipErrorInvalidValue;
    return values.f32 ? launch_spmv<float>(pl, row_ptr, col_idx, values.p, rows, v, out, pown, dot_out, ws, s, gate, ts)
                      : launch_spmv<double>(pl, row_ptr, col_idx, values.p, rows, v, out, pown, dot_out, ws, s, gate, ts);
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_spmv() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_spmv_csr_f64<double, 8, 1>));
}

}  // namespace cgx
