// cgx_bsmv.hip -- the block sparse matVec of a block-valued cgx_create_csr
// context (cgx_set_bsr): k_bsr_mult_f64, its plan rule, the one-time re-lay of
// the values and the two one-time extraction kernels of the preconditioners, a
// code object of its own.
//
// One pass over a BSR matrix (brow_ptr int64[nb + 1], bcol_idx int32[nnzb],
// values double[nnzb * BS * BS]) times one vector, out = A v, fp64, n = nb BS.
// Every stored block is dense BS x BS, 2 <= BS <= 8: an entry streams
// 8 + 4 / BS^2 bytes in place of CSR's 12, and a block reads its BS vector
// elements as one contiguous piece in place of BS^2 gathers.
//
// CSR-vector form on block rows.  T consecutive lanes own one block row
// (T = 2 .. 64), a wave covers 64 / T consecutive block rows, waves walk the
// groups with a grid stride as k_csr_mult_f64 does (cgx_csr_core.h).  Sub-lane
// l of block row I takes the blocks s+l, s+l+T, ... of [s, e) =
// [brow_ptr[I], brow_ptr[I+1]); for a block in block column c it reads
// v[c BS .. c BS + BS - 1] (16-byte loads when BS is even: c BS is even, v is
// 16-byte aligned) and holds BS accumulators.
//
// Device layout of the values.  A lane that read its own contiguous block
// would make every load instruction of the wave strided by BS^2 * 8 bytes.
// The values therefore lie in tiles of 64 consecutive blocks, entry-major
// inside a tile: entry e = i BS + j of block q at
//     ((q / 64) * BS^2 + e) * 64 + q % 64
// so the 64 lanes of a wave, which hold (runs of) consecutive blocks, read
// (runs of) consecutive doubles per load instruction -- cgx_pcg_block.hip's W
// is entry-major for the same reason.  The buffer holds
// ceil(nnzb / 64) * 64 * BS^2 doubles (bsr_tiled_count); k_bsr_tile_f64 re-lays
// the host layout (block after block, row-major inside one) once and zeroes the
// pad of the last tile, which no lane reads.  Measured (tools/bsmv_ab.py against
// tools/microbench/bsmv_plain.hip), the plain layout is not the
// slower one: best plan against best plan it is 1.19x faster at BS = 3 on a
// 5-blocks-per-row matrix, 1.08x on a 27-per-row one, level at BS = 4 -- a
// lane's block is whole cache lines that its BS^2 loads consume out of L1.
// The tiled layout stays because the kernel-level ABI names it; DESIGN.md
// lists the move to the plain layout as the next step.
//
// Summation order (a contract, include/cgx.h "Block storage";
// tests/_bsmv_order.py states it on the CPU).  For scalar row I BS + i:
// sub-lane l starts from +0.0 and, for each of its blocks in stored order and
// j = 0 .. BS-1 ascending inside a block, does acc_i = fma(B[i][j], v[c BS + j],
// acc_i); the T partial sums are combined as v[l] += v[l ^ o] for o = T/2,
// ..., 1.  Block columns need not be sorted, a duplicate block column is two
// terms, a stored zero is a term.  A row's sum depends on (BS, T) only: not on
// the load policy, the grid, the trips in flight, the row's place in a wave or
// the device layout.  An empty block row gives BS values of +0.0.
//
// The fused p.Ap goes through store_row / grid_sum_last_block_n<1> as in the CSR
// kernel; the storing lane adds its BS rows in ascending order.
//
// The kernel does not range-check bcol_idx: every host path checks the
// structure first (cgx_bsr_check).  No atomics, no spin-waits: plain vector
// loads and stores and __shfl_xor (the reduction hand-off is cgx_device.h's).
#include <algorithm>

#include "cgx_matvec_core.h"

namespace cgx {
namespace {

// Block trips a sub-lane has in flight: the loads of U trips (BS^2 values, the
// index, then the BS vector elements) are issued before their FMAs, which run
// in trip order.  A trip holds BS^2 + BS doubles: 12, 24, 40 registers at
// BS = 2, 3, 4, up to 144 at BS = 8, so U shrinks as BS grows (make asm: no
// instantiation uses scratch; the register table is in DESIGN.md s3).
template <int BS>
constexpr int kBsmvU = BS == 2 ? 4 : BS <= 4 ? 2 : 1;

template <int BS, int T, int NT>
__global__ __launch_bounds__(kNT) void k_bsr_mult_f64(const int64_t *__restrict__ brow_ptr,
                                                       const int32_t *__restrict__ bcol_idx,
                                                       const double *__restrict__ tiled, int64_t nb,
                                                       const double *__restrict__ v, double *__restrict__ out,
                                                       const double *__restrict__ pown, double *dot_out,
                                                       double *partials, unsigned *ticket, const int64_t *gate,
                                                       int64_t *ts) {
    if (gate && *gate) return;  // the solve stopped in an earlier iteration (device-side gating)
    ts_start(ts);
    constexpr int RW = 64 / T;  // block rows per wave
    constexpr int U = kBsmvU<BS>;
    constexpr int E = BS * BS;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int sub = lane & (T - 1), rloc = lane / T;
    const int64_t ngroups = (nb + RW - 1) / RW;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    double dacc[1] = {0.0};
    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t I = g * RW + rloc;
        const bool live = I < nb;  // block rows past the end: no loads, no store
        int64_t s = 0, e = 0;
        if (live) {
            s = brow_ptr[I];
            e = brow_ptr[I + 1];
        }
        double acc[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) acc[i] = 0.0;
        for (int64_t k = s + sub; k < e; k += (int64_t)U * T) {
            double a[U][E];
            double x[U][BS];
            int32_t c[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t q = k + (int64_t)u * T;
                const bool ok = q < e;
                c[u] = ok ? load_a<NT>(bcol_idx + q) : -1;
                const double *ap = tiled + ((q >> 6) * E) * 64 + (q & 63);
#pragma unroll
                for (int m = 0; m < E; ++m) a[u][m] = ok ? load_a<NT>(ap + m * 64) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double *vp = v + (int64_t)(c[u] >= 0 ? c[u] : 0) * BS;
                if constexpr (BS % 2 == 0) {
#pragma unroll
                    for (int j = 0; j < BS; j += 2) {
                        const d2 t = c[u] >= 0 ? *reinterpret_cast<const d2 *>(vp + j) : d2{0.0, 0.0};
                        x[u][j] = t.x;
                        x[u][j + 1] = t.y;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < BS; ++j) x[u][j] = c[u] >= 0 ? vp[j] : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (c[u] >= 0) {
#pragma unroll
                    for (int i = 0; i < BS; ++i)
#pragma unroll
                        for (int j = 0; j < BS; ++j) acc[i] = __builtin_fma(a[u][i * BS + j], x[u][j], acc[i]);
                }
        }
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int o = T / 2; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o, 64);
        if (live && sub == 0) {
#pragma unroll
            for (int i = 0; i < BS; ++i) store_row(I * BS + i, acc[i], out, pown, dacc[0]);
        }
    }
    if (pown) grid_sum_last_block_n<1>(dacc, partials, ticket, dot_out, 1u);
    ts_end(ts);
}

using BsrFn = decltype(&k_bsr_mult_f64<2, 8, 1>);  // the same type at every (BS, T, policy)

template <int BS, int NT>
BsrFn pick_bsr_t(int T) {
    switch (T) {
        case 2: return k_bsr_mult_f64<BS, 2, NT>;
        case 4: return k_bsr_mult_f64<BS, 4, NT>;
        case 8: return k_bsr_mult_f64<BS, 8, NT>;
        case 16: return k_bsr_mult_f64<BS, 16, NT>;
        case 32: return k_bsr_mult_f64<BS, 32, NT>;
        case 64: return k_bsr_mult_f64<BS, 64, NT>;
        default: return nullptr;
    }
}
template <int NT>
BsrFn pick_bsr_nt(int bs, int T) {
    switch (bs) {
        case 2: return pick_bsr_t<2, NT>(T);
        case 3: return pick_bsr_t<3, NT>(T);
        case 4: return pick_bsr_t<4, NT>(T);
        case 5: return pick_bsr_t<5, NT>(T);
        case 6: return pick_bsr_t<6, NT>(T);
        case 7: return pick_bsr_t<7, NT>(T);
        case 8: return pick_bsr_t<8, NT>(T);
        default: return nullptr;
    }
}
// The instantiated plan's kernel, or nullptr: block size 2..8, T lanes per block row, load policy 2 or 8.
BsrFn pick_bsr(int bs, int T, int nt) {
    return nt == 8 ? pick_bsr_nt<1>(bs, T) : nt == 2 ? pick_bsr_nt<0>(bs, T) : nullptr;
}

// tiled[t] for every slot t of the tiled buffer: the entry of the host layout it holds, +0.0 in the last tile's pad.
__global__ __launch_bounds__(kNT) void k_bsr_tile_f64(int64_t nnzb, int E, int64_t slots,
                                                      const double *__restrict__ values,
                                                      double *__restrict__ tiled) {
    for (int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x; t < slots; t += (int64_t)gridDim.x * kNT) {
        const int64_t q = (t / (64 * (int64_t)E)) * 64 + (t & 63);
        const int m = (int)((t >> 6) % E);
        tiled[t] = q < nnzb ? values[q * E + m] : 0.0;
    }
}

// One-time set-up, one scalar row per lane, on the host layout of the values:
// what k_csr_diag_minv (cgx_pcg.hip) gives on the expanded matrix bit for bit.
// The expansion lists row I bs + i's entries block after block in stored order,
// j ascending inside a block, so the row's entries in column I bs + i are
// B[i][i] of its blocks in block column I, in stored order, stored zeros
// included.
__global__ __launch_bounds__(kNT) void k_bsr_diag_minv(int64_t n, int bs, const int64_t *__restrict__ brow_ptr,
                                                       const int32_t *__restrict__ bcol_idx,
                                                       const double *__restrict__ values, double *__restrict__ minv,
                                                       unsigned long long *bad) {
#pragma clang fp contract(off)
    for (int64_t r = (int64_t)blockIdx.x * kNT + threadIdx.x; r < n; r += (int64_t)gridDim.x * kNT) {
        const int64_t I = r / bs;
        const int i = (int)(r - I * bs);
        double d = 0.0;
        bool found = false;
        const int64_t e1 = brow_ptr[I + 1];
        for (int64_t q = brow_ptr[I]; q < e1; ++q)
            if ((int64_t)bcol_idx[q] == I) {
                d = d + values[(q * bs + i) * bs + i];
                found = true;
            }
        const bool good = found && d > 0.0 && d < __builtin_inf();
        minv[r] = good ? 1.0 / d : found ? d : -0.0;
        if (!good) atomicMin(bad, (unsigned long long)r);
    }
}

// ... and what k_csr_diag_blocks (cgx_pcg_block.hip) gives on the expanded
// matrix, for any preconditioner block size pbs (not only pbs == bs): one
// scalar row per lane over the nblk * pbs rows of the diagonal blocks, the
// row's entries taken block after block in stored order, j ascending.
__global__ __launch_bounds__(kNT) void k_bsr_diag_blocks(int64_t n, int bs, int pbs, int64_t rows,
                                                         const int64_t *__restrict__ brow_ptr,
                                                         const int32_t *__restrict__ bcol_idx,
                                                         const double *__restrict__ values, double *__restrict__ D) {
#pragma clang fp contract(off)
    constexpr int kMaxBs = 8;
    for (int64_t r = (int64_t)blockIdx.x * kNT + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kNT) {
        const int64_t row0 = (r / pbs) * pbs;
        double d[kMaxBs];
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j) d[j] = 0.0;
        if (r < n) {
            const int64_t I = r / bs;
            const int i = (int)(r - I * bs);
            const int64_t e1 = brow_ptr[I + 1];
            for (int64_t q = brow_ptr[I]; q < e1; ++q) {
                const int64_t c0 = (int64_t)bcol_idx[q] * bs - row0;
                for (int jj = 0; jj < bs; ++jj) {
                    const int64_t c = c0 + jj;
                    const double val = values[(q * bs + i) * bs + jj];
#pragma unroll
                    for (int j = 0; j < kMaxBs; ++j) d[j] = (c == j) ? d[j] + val : d[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxBs; ++j)
            if (j < pbs) D[r * pbs + j] = d[j];
    }
}

}  // namespace

bool spmv_bsr_plan_ok(int bs, int T, int nt) { return pick_bsr(bs, T, nt) != nullptr; }

// T <= 0 / nt < 0 / blocks_per_cu <= 0 pick the defaults.
MatvecPlan plan_spmv_bsr(int device, int64_t nb, int64_t nnzb, int bs, int T, int nt, int blocks_per_cu) {
    MatvecPlan pl;
    pl.csr = 1;
    pl.bsr = bs;
    pl.U = 1;
    // Measured on MI355X, every (T, policy) interleaved in five rounds in one
    // process (tools/bsmv_ab.py, profiles/bsmv_ab_*.jsonl; ms per launch,
    // round-to-round spread below 1.7 %), T = 2 / 4 / 8 / 16 / 32 / 64:
    //   block 5-point grid, 1.44 M block rows, mean 5 blocks per block row
    //     bs = 3 (0.52 GB of values), policy 2: 0.165 / 0.137 / 0.144 / 0.233 /
    //     0.407 / 0.762; policy 8: 0.229 / 0.153 / 0.143 / 0.248 / 0.445 / 0.842
    //     bs = 4 (0.92 GB), policy 2: 0.309 / 0.230 / 0.233 / 0.348 / 0.611 /
    //     1.151; policy 8: 0.463 / 0.324 / 0.262 / 0.405 / 0.697 / 1.303
    //   block banded, 2^18 block rows, 27 blocks per full block row, bs = 3
    //     (0.51 GB), policy 2: 0.562 / 0.272 / 0.153 / 0.119 / 0.118 / 0.178;
    //     policy 8: 0.656 / 0.360 / 0.218 / 0.134 / 0.122 / 0.195
    // The CSR rule carried over -- T <= mean / (trips in flight), T = 2 and 8
    // here -- ran at 0.83x, 0.74x and 0.77x of the best plan: a block trip
    // already holds bs^2 loads, so a sub-lane needs no second block to keep
    // loads in flight, and more lanes per block row beat more block rows per
    // wave.  So T = the largest instantiated T <= the mean blocks per block row,
    // at least 2 (T = 4 and 16 here: the best plan, and 0.4 % behind it).  Means
    // other than 5 and 27, block sizes other than 3 and 4 and skewed block rows
    // are not measured.  Default-policy loads are faster or level at every T on
    // all three: policy 2 at every size.
    // nnzb < 0 (the kernel-level call, which does not know it): T = 8.
    int t = 8;
    if (nnzb >= 0 && nb > 0) {
        const int64_t mean = nnzb / nb;
        for (t = 2; t < 64 && 2 * t <= mean;) t *= 2;
    }
    pl.R = 64 / t;
    pl.nt = 2;
    // CGX_BSMV_PLAN = "T=..,nt=..,bpc=..": taken when it names an instantiated plan, then the arguments
    const char *env = "CGX_BSMV_PLAN";
    const int eT = env_opt(env, "T", t), en = env_opt(env, "nt", pl.nt);
    if (spmv_bsr_plan_ok(bs, eT, en)) pl.R = 64 / eT, pl.nt = en;
    if (T > 0) pl.R = spmv_bsr_plan_ok(bs, T, 8) ? 64 / T : 0;
    if (nt >= 0) pl.nt = nt;
    if (pl.R < 1 || !spmv_bsr_plan_ok(bs, 64 / pl.R, pl.nt)) pl.R = 64 / t, pl.nt = 2;
    pl.blocks = plan_grid(reinterpret_cast<const void *>(pick_bsr(bs, 64 / pl.R, pl.nt)), device, nb, pl.R, 8, env,
                          blocks_per_cu);
    return pl;
}

hipError_t spmv_bsr_f64(const MatvecPlan &pl, int bs, const int64_t *brow_ptr, const int32_t *bcol_idx,
                        const double *tiled, int64_t nb, const double *v, double *out, const double *pown,
                        double *dot_out, const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    if (nb <= 0) return hipSuccess;
    if (!pl.csr || pl.bsr != bs || pl.R < 1 || pl.R > 32 || !spmv_bsr_plan_ok(bs, 64 / pl.R, pl.nt) ||
        pl.blocks < 1 || pl.blocks > kMaxRedBlocks)
        return hipErrorInvalidValue;
    if (bs % 2 == 0 && !al16(v)) return hipErrorInvalidValue;  // the 16-byte loads of v
    hipLaunchKernelGGL(pick_bsr(bs, 64 / pl.R, pl.nt), dim3(pl.blocks), dim3(kNT), 0, s, brow_ptr, bcol_idx, tiled, nb,
                       v, out, pown, dot_out, ws.partials, ws.tickets + T_MATVEC, gate, ts);
    return hipGetLastError();
}

hipError_t bsr_tile_values_f64(int64_t nnzb, int bs, const double *values, double *tiled, hipStream_t s) {
    if (bs < 2 || bs > kMaxBsrBlock || nnzb < 0) return hipErrorInvalidValue;
    if (nnzb == 0) return hipSuccess;
    const int64_t slots = bsr_tiled_count(nnzb, bs);
    hipLaunchKernelGGL(k_bsr_tile_f64, dim3(grid_1d(slots, kNT, 65536)), dim3(kNT), 0, s, nnzb, bs * bs, slots, values,
                       tiled);
    return hipGetLastError();
}

hipError_t bsr_diag_minv_f64(int64_t n, int bs, const int64_t *brow_ptr, const int32_t *bcol_idx, const double *values,
                             double *minv, unsigned long long *bad, hipStream_t s) {
    if (bs < 2 || bs > kMaxBsrBlock || n < 1 || n % bs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bsr_diag_minv, dim3(grid_1d(n, kNT, 65536)), dim3(kNT), 0, s, n, bs, brow_ptr, bcol_idx, values,
                       minv, bad);
    return hipGetLastError();
}

hipError_t bsr_diag_blocks_f64(int64_t n, int bs, int pbs, const int64_t *brow_ptr, const int32_t *bcol_idx,
                               const double *values, double *D, hipStream_t s) {
    if (bs < 2 || bs > kMaxBsrBlock || pbs < 2 || pbs > kMaxPcBlock || n < 1 || n % bs) return hipErrorInvalidValue;
    const int64_t rows = (n + pbs - 1) / pbs * pbs;
    hipLaunchKernelGGL(k_bsr_diag_blocks, dim3(grid_1d(rows, kNT, 65536)), dim3(kNT), 0, s, n, bs, pbs, rows, brow_ptr,
                       bcol_idx, values, D);
    return hipGetLastError();
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_bsmv() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_bsr_mult_f64<2, 8, 0>));
}

}  // namespace cgx
