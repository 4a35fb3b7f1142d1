// cgx_dia_sym.hip -- the one-sided diagonal matVec of a symmetric A held by the
// diagonals of its upper triangle (cgx_set_dia_sym): k_dia_sym_mult_f64, its
// plan rule and the one-time extraction of the block preconditioner's blocks, a
// code object of its own.  The kernel is cgx_dia_core.h's walk (rows per lane,
// groups, the 16-byte loads, the fused p.Ap) over the terms below.
//
// Storage: scipy's dia_matrix of triu(A).  offsets int32[ndiag], 0 <= o < n,
// data double[ndiag * ld], data[k * ld + j] = A[j - o][j] for j in [o, n).  The
// stored diagonal of offset o > 0 also stands for the diagonal -o:
// A[j][j - o] = A[j - o][j].  So row i takes from diagonal k
//     upper  data[k][i + o] * v[i + o]   where i + o < n   (o > 0 only)
//     lower  data[k][i]     * v[i - o]   where i - o >= 0
// and a diagonal of offset 0 is its lower term alone.  Every value is used
// twice, o rows apart: the matrix streams 8 ndiag_stored + 16 bytes per row from
// memory when the second use still finds its line on the die.  The upper piece
// (the first use in the walk's order) is a default-policy load, the lower piece
// (the last use; all of an offset-0 diagonal) takes the plan's policy, 2 or 8.
// With R = 2 the lower data piece is always one 16-byte load (even pitch,
// aligned base, i even); the upper data piece and both v pieces are when o is
// even.
//
// Range rule.  A group of rows is interior when both terms of every stored
// diagonal reach every one of its rows, g0 - omax >= 0 and
// g0 + 64 R - 1 + omax < n.  In the other groups the slot is clamped into the
// diagonal's own range [o, n) and the vector index into [0, n).  Nothing is read
// outside v[0 .. n) or outside a diagonal's slots [o, n), and a NaN in an unused
// slot never reaches an accumulator.  An unchecked offset of the kernel-level
// call (o < 0 or o >= n) adds no term and reads nothing outside the arrays: a
// negative one sends every group down the clamped path.
//
// Summation order (a contract, include/cgx.h "One-sided diagonal storage";
// tests/_dia_sym.py states it on the CPU).  Row i starts from +0.0 and, for
// k = 0 .. ndiag-1 in stored order, does the upper term, then the lower term,
// each acc = fma(a, x, acc) where it exists: one accumulator per row, no
// cross-lane combine.  That is, bit for bit, k_dia_mult_f64 on the expansion
// (every stored o > 0 as the two consecutive diagonals o, -o), the fused p.Ap
// included at the same R and grid.  A row's sum depends on nothing but the
// matrix and v: not on R, U, the load policy, the grid or the pitch.
#include <algorithm>

#include "cgx_dia_core.h"

namespace cgx {
namespace {

// A stored diagonal and its mirror: up to two terms per stored diagonal and row.
struct SymTerms {
    // U stored diagonals from k0 on, both terms of each in range for every row of the
    // lane (0 <= o <= i0, i0 + R - 1 + o < n): loads, then FMAs in the contract's order.
    template <int R, int U, int NT>
    static __device__ __forceinline__ void interior(const int32_t *__restrict__ offsets,
                                                    const double *__restrict__ data, int64_t ld,
                                                    const double *__restrict__ v, int64_t i0, int64_t k0, bool vec,
                                                    double (&acc)[R]) {
        double au[U][R], xu[U][R], al[U][R], xl[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t o = offsets[k0 + u];
            const double *row = data + (k0 + u) * ld + i0;
            const bool even = vec && !(o & 1);
            if (o > 0) load_piece<R, 0>(row + o, even, au[u]);  // first use: the line stays on the die
            load_piece<R, NT>(row, vec, al[u]);                 // last use
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t o = offsets[k0 + u];
            const bool even = vec && !(o & 1);
            if (o > 0) load_piece<R, 0>(v + i0 + o, even, xu[u]);
            load_piece<R, 0>(v + i0 - o, even, xl[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool up = offsets[k0 + u] > 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (up) acc[r] = __builtin_fma(au[u][r], xu[u][r], acc[r]);
                acc[r] = __builtin_fma(al[u][r], xl[u][r], acc[r]);
            }
        }
    }

    // U stored diagonals from k0 on for one row that a term may miss (or that is past
    // the end): slots clamped into [o, n), vector indices into [0, n), 8-byte loads,
    // the terms selected away.
    template <int U, int NT>
    static __device__ __forceinline__ void guarded(const int32_t *__restrict__ offsets,
                                                   const double *__restrict__ data, int64_t ld,
                                                   const double *__restrict__ v, int64_t n, int64_t i, int64_t k0,
                                                   double &acc) {
        double au[U], xu[U], al[U], xl[U];
        bool oku[U], okl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t o = offsets[k0 + u];
            const bool valid = o >= 0 && o < n && i < n;  // an unchecked offset of the kernel-level call adds no term
            oku[u] = valid && o > 0 && i + o < n;
            okl[u] = valid && i - o >= 0;
            const int64_t lo = o < 0 ? 0 : o > n - 1 ? n - 1 : o;  // the first slot of the diagonal, inside the array
            int64_t ju = i + o;  // the upper term's slot and vector index
            ju = ju < lo ? lo : ju > n - 1 ? n - 1 : ju;
            int64_t jl = i;  // the lower term's slot ...
            jl = jl < lo ? lo : jl > n - 1 ? n - 1 : jl;
            int64_t jv = jl - o;  // ... and its vector index
            jv = jv < 0 ? 0 : jv > n - 1 ? n - 1 : jv;
            const double *row = data + (k0 + u) * ld;
            au[u] = load_a<0>(row + ju);
            xu[u] = v[ju];
            al[u] = load_a<NT>(row + jl);
            xl[u] = v[jv];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double t = __builtin_fma(au[u], xu[u], acc);
            acc = oku[u] ? t : acc;
            const double w = __builtin_fma(al[u], xl[u], acc);
            acc = okl[u] ? w : acc;
        }
    }

    // both terms of every diagonal reach every row (omin < 0: an unchecked offset)
    static __device__ __forceinline__ bool is_interior(int64_t g0, int RW, int64_t omin, int64_t omax, int64_t n) {
        return omin >= 0 && g0 - omax >= 0 && g0 + RW - 1 + omax < n;
    }
};

template <int R, int U, int NT>
__global__ __launch_bounds__(kNT) void k_dia_sym_mult_f64(const int32_t *__restrict__ offsets,
                                                           const double *__restrict__ data, int64_t ld, int64_t n,
                                                           int64_t ndiag, int vec, const double *__restrict__ v,
                                                           double *__restrict__ out, const double *__restrict__ pown,
                                                           double *dot_out, double *partials, unsigned *ticket,
                                                           const int64_t *gate, int64_t *ts) {
    dia_walk<SymTerms, R, U, NT>(offsets, data, ld, n, ndiag, vec, v, out, pown, dot_out, partials, ticket, gate, ts);
}

struct SymKernels {
    template <int R, int U, int NT>
    static DiaFn fn() { return k_dia_sym_mult_f64<R, U, NT>; }
};
using Host = DiaHost<SymKernels>;

// One-time set-up, one row per lane over the nblk * pbs rows of the diagonal
// blocks: what k_csr_diag_blocks (cgx_pcg_block.hip) gives on the expansion bit
// for bit.  Row r's entries are, per stored k in stored order, (r + o,
// data[k][r + o]) then (r - o, data[k][r]) for o > 0 and (r, data[k][r]) for
// o = 0; D_b[i][j] is the sum from +0.0 of those in column j of the block.
__global__ __launch_bounds__(kNT) void k_dia_sym_diag_blocks(int64_t n, int pbs, int64_t rows, int64_t ndiag,
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
                const int64_t o = offsets[k];
                if (o < 0 || o >= n) continue;
                const int64_t cu = r + o - row0, cl = r - o - row0;  // the two terms' columns inside the block
                if (o > 0 && r + o < n && cu < pbs) {  // cu >= 0 as o > 0
                    const double val = data[k * ld + r + o];
#pragma unroll
                    for (int j = 0; j < kMaxBs; ++j) d[j] = (cu == j) ? d[j] + val : d[j];
                }
                if (cl >= 0) {  // r - o >= row0 >= 0, and cl < pbs as o >= 0
                    const double val = data[k * ld + r];
#pragma unroll
                    for (int j = 0; j < kMaxBs; ++j) d[j] = (cl == j) ? d[j] + val : d[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j)
            if (j < pbs) D[r * pbs + j] = d[j];
    }
}

}  // namespace

bool spmv_dia_sym_plan_ok(int R, int U, int nt) { return Host::plan_ok(R, U, nt); }

// R / U <= 0, nt < 0, blocks_per_cu <= 0 pick the defaults (the rule is DiaHost::plan's, under CGX_DIA_SYM_PLAN).
MatvecPlan plan_spmv_dia_sym(int device, int64_t n, int64_t ndiag, int R, int U, int nt, int blocks_per_cu) {
    // Measured on MI355X, every (R, U, policy) interleaved in five rounds in one
    // process with k_dia_mult_f64's plans on the full matrix (tools/dia_sym_ab.py,
    // profiles/dia_sym_ab_*.jsonl; ms per launch, round-to-round spread 2.0 % on
    // the first matrix, 6.1 % on the second), U = 1 / 2 / 4 / 8:
    //   5-point Poisson, m = 4096 (16.8 M rows, 3 stored diagonals of 5)
    //     R = 1, policy 2: 0.223 / 0.201 / 0.225 / 0.210; policy 8: 0.225 / 0.207 /
    //     0.231 / 0.212;  R = 2, policy 2: 0.148 / 0.142 / 0.130 / 0.133; policy 8:
    //     0.155 / 0.150 / 0.141 / 0.140
    //   banded, n = 2^20, 33 stored diagonals of 65
    //     R = 1, policy 2: 0.148 / 0.100 / 0.097 / 0.091; policy 8: 0.140 / 0.097 /
    //     0.093 / 0.088;  R = 2, policy 2: 0.078 / 0.064 / 0.069 / 0.061; policy 8:
    //     0.087 / 0.072 / 0.076 / 0.066
    // (k_dia_mult_f64's best plan on the full matrices in the same rounds: 0.153
    // and 0.119).  Unlike the full kernel this one gains from two rows per lane
    // (1.5x on both matrices: it issues a load per term, as many as the full kernel,
    // and the 16-byte loads halve them) and from more diagonals in flight.  Two rows
    // per lane, 8 stored diagonals in flight, default policy on the last use too is
    // the best plan on the banded matrix and 2.1 % behind the best (U = 4) on the
    // Poisson matrix, where 3 stored diagonals never fill a trip of 8, so it is the
    // default at every size.  The non-temporal policy on the last use loses 5-8 %
    // at R = 2.  Stored counts other than 3 and 33 are not measured.
    (void)ndiag;
    return Host::plan(device, n, R, U, nt, blocks_per_cu, /*r0=*/2, /*u0=*/8, /*n0=*/2, "CGX_DIA_SYM_PLAN", /*pl.dia=*/2);
}

hipError_t spmv_dia_sym_f64(const MatvecPlan &pl, const int32_t *offsets, const double *data, int64_t ld, int64_t n,
                            int64_t ndiag, const double *v, double *out, const double *pown, double *dot_out,
                            const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    return Host::launch(pl, 2, offsets, data, ld, n, ndiag, v, out, pown, dot_out, ws, s, gate, ts);
}

hipError_t dia_sym_diag_blocks_f64(int64_t n, int pbs, int64_t ndiag, const int32_t *offsets, const double *data,
                                   int64_t ld, double *D, hipStream_t s) {
    if (pbs < 2 || pbs > kMaxPcBlock || n < 1 || ndiag < 0 || ld < n) return hipErrorInvalidValue;
    const int64_t rows = (n + pbs - 1) / pbs * pbs;
    hipLaunchKernelGGL(k_dia_sym_diag_blocks, dim3(grid_1d(rows, kNT, 65536)), dim3(kNT), 0, s, n, pbs, rows, ndiag,
                       offsets, data, ld, D);
    return hipGetLastError();
}

hipError_t preload_dia_sym() { return Host::preload(); }

}  // namespace cgx
