// cgx_dia.hip -- the diagonal-storage matVec of a diagonal-valued cgx_create_csr
// context (cgx_set_dia): k_dia_mult_f64, its plan rule and the two one-time
// extraction kernels of the preconditioners, a code object of its own.
//
// One pass over a matrix held by diagonals (scipy's dia_matrix, square:
// offsets int32[ndiag], data double[ndiag * ld], data[k * ld + j] =
// A[j - offsets[k]][j]) times one vector, out = A v, fp64.  There are no column
// indices and no gathers: row i on the diagonal of offset o multiplies
// data[k * ld + i + o] by v[i + o], both contiguous across a wave.  An entry
// streams 8 bytes in place of CSR's 12, a row 8 ndiag + 16 in place of
// 12 L + 24.
//
// The kernel is cgx_dia_core.h's walk (rows per lane, groups, the fused p.Ap)
// over the terms below.  With R = 2 a diagonal of even offset loads data and v
// with 16-byte loads (i + o is even), an odd offset takes 8-byte loads.  data is
// read once (load_a: default policy or non-temporal), v is the only reused data
// (default policy).
//
// Range rule.  A group of rows is interior when every diagonal reaches every
// one of its rows,
//     g0 + min(0, min o) >= 0  and  g0 + 64 R - 1 + max(0, max o) < n.
// In the other groups (the first and last max |o| rows, a partial last group)
// the column is clamped into the diagonal's own range [max(0, o), min(n, n + o)).
// So nothing is read outside v[0 .. n) or outside the slots of a diagonal that
// hold an entry of A, and a NaN in an unused slot never reaches an accumulator.
//
// Summation order (a contract, include/cgx.h "Diagonal storage";
// tests/_dia_order.py states it on the CPU).  Row i starts from +0.0 and, for
// k = 0 .. ndiag-1 in stored order where 0 <= i + offsets[k] < n, does
// acc = fma(data[k][i + o], v[i + o], acc): one accumulator per row, no
// cross-lane combine.  Diagonals need not be sorted, a duplicate offset is two
// terms, a stored zero is a term.  A row's sum depends on nothing but the
// matrix and v: not on R, U, the load policy, the grid or the pitch.  A row no
// diagonal reaches gives +0.0.
#include <algorithm>

#include "cgx_dia_core.h"

namespace cgx {
namespace {

// Every diagonal as stored: one term per diagonal and row.
struct FullTerms {
    // U diagonals from k0 on, every row of the lane in range: loads (data, then v), then FMAs in stored order.
    template <int R, int U, int NT>
    static __device__ __forceinline__ void interior(const int32_t *__restrict__ offsets,
                                                    const double *__restrict__ data, int64_t ld,
                                                    const double *__restrict__ v, int64_t i0, int64_t k0, bool vec,
                                                    double (&acc)[R]) {
        double a[U][R], x[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t o = offsets[k0 + u];
            load_piece<R, NT>(data + (k0 + u) * ld + o + i0, vec && !(o & 1), a[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t o = offsets[k0 + u];
            load_piece<R, 0>(v + o + i0, vec && !(o & 1), x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_fma(a[u][r], x[u][r], acc[r]);
    }

    // U diagonals from k0 on for one row that some diagonal may miss (or that is
    // past the end): the column clamped into the diagonal's range, 8-byte loads,
    // the term selected away.
    template <int U, int NT>
    static __device__ __forceinline__ void guarded(const int32_t *__restrict__ offsets,
                                                   const double *__restrict__ data, int64_t ld,
                                                   const double *__restrict__ v, int64_t n, int64_t i, int64_t k0,
                                                   double &acc) {
        double a[U], x[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t o = offsets[k0 + u];
            const int64_t j = i + o;
            const int64_t lo = o > 0 ? o : 0, hi = (o < 0 ? n + o : n) - 1;  // the diagonal's columns, lo <= hi as |o| < n
            ok[u] = i < n && j >= lo && j <= hi;
            int64_t jc = j < lo ? lo : j > hi ? hi : j;
            jc = jc < 0 ? 0 : jc >= n ? n - 1 : jc;  // an unchecked offset of the kernel-level call stays inside the arrays
            a[u] = load_a<NT>(data + (k0 + u) * ld + jc);
            x[u] = v[jc];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double t = __builtin_fma(a[u], x[u], acc);
            acc = ok[u] ? t : acc;
        }
    }

    // every diagonal reaches every row of the group
    static __device__ __forceinline__ bool is_interior(int64_t g0, int RW, int64_t omin, int64_t omax, int64_t n) {
        return g0 + omin >= 0 && g0 + RW - 1 + omax < n;
    }
};

template <int R, int U, int NT>
__global__ __launch_bounds__(kNT) void k_dia_mult_f64(const int32_t *__restrict__ offsets,
                                                       const double *__restrict__ data, int64_t ld, int64_t n,
                                                       int64_t ndiag, int vec, const double *__restrict__ v,
                                                       double *__restrict__ out, const double *__restrict__ pown,
                                                       double *dot_out, double *partials, unsigned *ticket,
                                                       const int64_t *gate, int64_t *ts) {
    dia_walk<FullTerms, R, U, NT>(offsets, data, ld, n, ndiag, vec, v, out, pown, dot_out, partials, ticket, gate, ts);
}

struct FullKernels {
    template <int R, int U, int NT>
    static DiaFn fn() { return k_dia_mult_f64<R, U, NT>; }
};
using Host = DiaHost<FullKernels>;

// One-time set-up, one row per lane: what k_csr_diag_minv (cgx_pcg.hip) gives
// on the expanded matrix bit for bit.  The expansion lists row i's entries
// diagonal after diagonal in stored order, so the row's entries in column i are
// data[k][i] of the diagonals of offset 0, in stored order, stored zeros
// included.
__global__ __launch_bounds__(kNT) void k_dia_diag_minv(int64_t n, int64_t ndiag, const int32_t *__restrict__ offsets,
                                                       const double *__restrict__ data, int64_t ld,
                                                       double *__restrict__ minv, unsigned long long *bad) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT) {
        double d = 0.0;
        bool found = false;
        for (int64_t k = 0; k < ndiag; ++k)
            if (offsets[k] == 0) {
                d = d + data[k * ld + i];
                found = true;
            }
        const bool good = found && d > 0.0 && d < __builtin_inf();
        minv[i] = good ? 1.0 / d : found ? d : -0.0;
        if (!good) atomicMin(bad, (unsigned long long)i);
    }
}

// ... and what k_csr_diag_blocks (cgx_pcg_block.hip) gives on the expanded
// matrix: one row per lane over the nblk * pbs rows of the diagonal blocks,
// D_b[i][j] the sum from +0.0 of the diagonals of offset j - i in stored order.
__global__ __launch_bounds__(kNT) void k_dia_diag_blocks(int64_t n, int pbs, int64_t rows, int64_t ndiag,
                                                         const int32_t *__restrict__ offsets,
                                                         const double *__restrict__ data, int64_t ld,
                                                         double *__restrict__ D) {
#pragma clang fp contract(off)
    constexpr int kMaxBs = 8;
    for (int64_t r = (int64_t)blockIdx.x * kNT + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kNT) {
        const int64_t row0 = (r / pbs) * pbs;
        double d[kMaxBs];
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j) d[j] = 0.0;
        if (r < n) {
            for (int64_t k = 0; k < ndiag; ++k) {
                const int64_t col = r + offsets[k], c = col - row0;
                if (col < 0 || col >= n || c < 0 || c >= pbs) continue;  // no entry of the row, or outside its block
                const double val = data[k * ld + col];
#pragma unroll
                for (int j = 0; j < kMaxBs; ++j) d[j] = (c == j) ? d[j] + val : d[j];
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j)
            if (j < pbs) D[r * pbs + j] = d[j];
    }
}

}  // namespace

bool spmv_dia_plan_ok(int R, int U, int nt) { return Host::plan_ok(R, U, nt); }

// R / U <= 0, nt < 0, blocks_per_cu <= 0 pick the defaults (the rule is DiaHost::plan's, under CGX_DIA_PLAN).
MatvecPlan plan_spmv_dia(int device, int64_t n, int64_t ndiag, int R, int U, int nt, int blocks_per_cu) {
    // Measured on MI355X, every (R, U, policy) interleaved in five rounds in one
    // process with k_csr_mult_f64's plans on the same matrix (tools/dia_ab.py,
    // profiles/dia_ab_*.jsonl; ms per launch, round-to-round spread below 0.9 %
    // on the first matrix, 4.7 % on the second), U = 1 / 2 / 4 / 8:
    //   5-point Poisson, m = 4096 (16.8 M rows, 5 diagonals, 0.67 GB of values)
    //     R = 1, policy 2: 0.174 / 0.211 / 0.204 / 0.250; policy 8: 0.160 / 0.193 /
    //     0.184 / 0.236;  R = 2, policy 2: 0.196 / 0.196 / 0.194 / 0.178; policy 8:
    //     0.173 / 0.171 / 0.167 / 0.158
    //   banded, n = 2^20, 65 diagonals (0.55 GB)
    //     R = 1, policy 2: 0.121 / 0.148 / 0.147 / 0.126; policy 8: 0.120 / 0.147 /
    //     0.144 / 0.123;  R = 2, policy 2: 0.134 / 0.131 / 0.131 / 0.131; policy 8:
    //     0.140 / 0.135 / 0.132 / 0.131
    // (the CSR kernel's best plan on the same matrices: 0.310 and 0.173).  One row
    // per lane with one diagonal in flight and non-temporal loads of the values is
    // the best plan on the banded matrix and 1.1 % behind the best (R = 2, U = 8,
    // policy 8, where 5 diagonals never fill a trip of 8) on the Poisson matrix, so
    // it is the default at every size: the rows of a wave are independent, 8 waves
    // per SIMD already keep the loads in flight, and more diagonals per trip cost
    // registers and scalar work without shortening any chain.  Why U = 2 and 4 are
    // 20 % slower than U = 1 at R = 1 has not been looked into.  Unlike the CSR
    // kernel the values gain from the non-temporal policy (8 % at 5 diagonals, level
    // at 65): nothing but v is read twice.  Diagonal counts other than 5 and 65 and
    // matrices below 0.5 GB are not measured.
    (void)ndiag;
    return Host::plan(device, n, R, U, nt, blocks_per_cu, /*r0=*/1, /*u0=*/1, /*n0=*/8, "CGX_DIA_PLAN", /*pl.dia=*/1);
}

hipError_t spmv_dia_f64(const MatvecPlan &pl, const int32_t *offsets, const double *data, int64_t ld, int64_t n,
                        int64_t ndiag, const double *v, double *out, const double *pown, double *dot_out,
                        const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    return Host::launch(pl, 1, offsets, data, ld, n, ndiag, v, out, pown, dot_out, ws, s, gate, ts);
}

hipError_t dia_diag_minv_f64(int64_t n, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld,
                             double *minv, unsigned long long *bad, hipStream_t s) {
    if (n < 1 || ndiag < 0 || ld < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dia_diag_minv, dim3(grid_1d(n, kNT, 65536)), dim3(kNT), 0, s, n, ndiag, offsets, data, ld, minv,
                       bad);
    return hipGetLastError();
}

hipError_t dia_diag_blocks_f64(int64_t n, int pbs, int64_t ndiag, const int32_t *offsets, const double *data,
                               int64_t ld, double *D, hipStream_t s) {
    if (pbs < 2 || pbs > kMaxPcBlock || n < 1 || ndiag < 0 || ld < n) return hipErrorInvalidValue;
    const int64_t rows = (n + pbs - 1) / pbs * pbs;
    hipLaunchKernelGGL(k_dia_diag_blocks, dim3(grid_1d(rows, kNT, 65536)), dim3(kNT), 0, s, n, pbs, rows, ndiag, offsets,
                       data, ld, D);
    return hipGetLastError();
}

hipError_t preload_dia() { return Host::preload(); }

}  // namespace cgx
