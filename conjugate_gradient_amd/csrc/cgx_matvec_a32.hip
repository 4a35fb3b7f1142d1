// cgx_matvec_a32.hip -- the dense matVec of CGX_A_F32: A stored as float,
// every operation in fp64.
//
// The reference holds A as float on every input path (fscanf("%f"), float *A,
// MPI_FLOAT); a float widens to double exactly, so out = A p computed here is
// the fp64 product of that same matrix at half the bytes k_matvec_f64 streams.
// No fp32 arithmetic: each a_ij is converted (v_cvt_f64_f32, exact) and
// multiplied by p_j with an fp64 FMA.
//
// cgx_matvec_core.h's skeleton with a float4 of A per lane: a chunk is 256
// columns, the p chunk a lane holds is four doubles (twice k_matvec_f64's per
// A byte), and a lane has four accumulators per row, summed ((x + y) + (z + w)).
#include "cgx_matvec_core.h"

#include <algorithm>
#include <iterator>

namespace cgx {
namespace {

// out[i] = sum_j (double)A[i*lda + j] * v[j]; vec_cols (a multiple of 256, 0
// when a pointer or the pitch is not 16-B aligned) columns go through the
// vector path, [vec_cols, cols) through the scalar tail.
template <int R, int U, int NT>
__global__ __launch_bounds__(kNT) void k_matvec_a32(const float *__restrict__ A, int64_t lda, int64_t rows,
                                                     int64_t cols, int64_t vec_cols, const double *__restrict__ v,
                                                     double *__restrict__ out, const double *__restrict__ pown,
                                                     double *dot_out, double *partials, unsigned *ticket,
                                                     const int64_t *gate, int64_t *ts) {
    if (gate && *gate) return;  // the solve converged in an earlier iteration (device-side gating)
    ts_start(ts);
    const int lane = threadIdx.x & 63;
    const VecPlain<d4> vec[1] = {vec_plain<d4>(v, lane)};
    double dacc = 0.0;
    for_row_groups<1, R, f4, d4>(A, lda, rows, [&](int64_t r0, const auto &ridx, const auto &arow, auto &acc) {
        chunks_pipe<NT, U>(arow, vec, 0, vec_cols >> 8, acc);
        tail_cols(A, lda, ridx, vec, lane, vec_cols, cols, acc);
        const double mine = row_sums(acc[0], lane);
        if (lane < R && r0 + lane < rows) store_row(r0 + lane, mine, out, pown, dacc);
    });
    if (pown) grid_sum_last_block(dacc, partials, ticket, dot_out);
    ts_end(ts);
}

using A32Fn = decltype(&k_matvec_a32<4, 4, 1>);

// The instantiated plans (cgx_set_matvec_plan accepts exactly these): rows per
// wave x 256-column chunks in flight, each with both load policies (2
// default-policy loads, 8 non-temporal).
constexpr struct { int R, U; } kA32Plans[] = {{1, 4}, {1, 8}, {2, 4}, {4, 2}, {4, 4}, {8, 2}};

// the listed plan's kernel, or nullptr
template <int NT, size_t I = 0>
A32Fn pick_a32_nt(int R, int U) {
    if constexpr (I == std::size(kA32Plans)) return nullptr;
    else return (kA32Plans[I].R == R && kA32Plans[I].U == U) ? k_matvec_a32<kA32Plans[I].R, kA32Plans[I].U, NT>
                                                             : pick_a32_nt<NT, I + 1>(R, U);
}
A32Fn pick_a32(int R, int U, int nt) {
    return nt == 8 ? pick_a32_nt<1>(R, U) : nt == 2 ? pick_a32_nt<0>(R, U) : nullptr;
}

}  // namespace

bool matvec_a32_plan_ok(int R, int U, int nt) { return pick_a32(R, U, nt) != nullptr; }

MatvecPlan plan_matvec_a32(int device, int64_t rows, int R, int U, int nt, int blocks_per_cu, int64_t cols) {
    MatvecPlan pl;
    pl.a32 = 1;
    const int cus = cu_count(device);
    // Measured on MI355X, every instantiated plan interleaved with the CGX_F64
    // default in the same rounds (profiles/a32_sweep_plans_n*.jsonl): the rate
    // rises with the rows per wave, i.e. as the p bytes read per byte of A
    // fall (R = 1 / 2 / 4 / 8 at N = 65536: 4.89 / 6.31 / 7.09 / 7.14 TB/s on
    // 4 N^2 + 16 N bytes; k_matvec_f64 in the same rounds 7.24).  R = 8, U = 2
    // is the best median at 65536^2 (2.405 against 2.424 ms for R = 4, U = 4),
    // R = 4, U = 4 at 16384^2 (0.1690 against 0.1700 ms), where eight rows per
    // wave leave a resident wave two row groups; in between is not measured,
    // and R = 8 is taken from four groups per resident wave up.  Both hold 16
    // KiB of A per step and wave, as k_matvec_f64's default; 256 VGPRs, one
    // wave per SIMD, no scratch.  Fewer rows per wave when there are too few
    // rows to give every resident wave a group.
    const int64_t want_waves = (int64_t)cus * 4;
    pl.R = rows >= 32 * want_waves ? 8 : rows >= 4 * want_waves ? 4 : rows >= 2 * want_waves ? 2 : 1;
    pl.U = pl.R == 8 ? 2 : 4;
    // an A of up to 64 MiB with default-policy loads, so it stays in the MALL
    // between iterations (as plan_matvec_f64)
    pl.nt = (cols > 0 && rows * cols * 4 <= (int64_t(64) << 20)) ? 2 : 8;
    // CGX_MV_A32_PLAN="R=..,U=..,nt=..,bpc=..": taken when it names an instantiated plan
    plan_listed(pl, "CGX_MV_A32_PLAN", R, U, nt, [](int, int r, int u, int n) { return matvec_a32_plan_ok(r, u, n); },
                4, 4);
    pl.blocks = plan_grid(reinterpret_cast<const void *>(pick_a32(pl.R, pl.U, pl.nt)), device, rows, pl.R, 2,
                          "CGX_MV_A32_PLAN", blocks_per_cu);
    return pl;
}

hipError_t matvec_a32(const MatvecPlan &pl, const float *A, int64_t lda, int64_t rows, int64_t cols, const double *v,
                      double *out, const double *pown, double *dot_out, const RedWs &ws, hipStream_t s,
                      const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    if (!pl.a32 || !matvec_a32_plan_ok(pl.R, pl.U, pl.nt) || pl.blocks < 1) return hipErrorInvalidValue;
    // The vector path needs 16-B-aligned rows and a 32-B-aligned p (a lane
    // reads four doubles); otherwise every column goes through the scalar tail.
    const int64_t vec_cols = matvec_vec_cols(
        (reinterpret_cast<uintptr_t>(A) & 15) | (reinterpret_cast<uintptr_t>(v) & 31), (lda & 3) == 0, cols, 256);
    hipLaunchKernelGGL(pick_a32(pl.R, pl.U, pl.nt), dim3(pl.blocks), dim3(kNT), 0, s, A, lda, rows, cols, vec_cols, v,
                       out, pown, dot_out, ws.partials, ws.tickets + T_MATVEC, gate, ts);
    return hipGetLastError();
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_matvec_a32() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_matvec_a32<4, 4, 1>));
}

}  // namespace cgx
