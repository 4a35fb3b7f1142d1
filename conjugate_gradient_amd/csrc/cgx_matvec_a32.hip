// cgx_matvec_a32.hip -- the dense matVec of CGX_A_F32: A stored as float,
// every operation in fp64.
//
// The reference holds A as float on every input path (fscanf("%f"), float *A,
// MPI_FLOAT); a float widens to double exactly, so out = A p computed here is
// the fp64 product of that same matrix at half the bytes k_matvec_f64 streams.
// No fp32 arithmetic: each a_ij is converted (v_cvt_f64_f32, exact) and
// multiplied by p_j with an fp64 FMA.
//
// Structure (k_matvec_f64's): 16-B-per-lane coalesced loads of A
// -- a float4 per lane, so a wave covers one 1-KiB, 256-column chunk of a row
// per instruction -- R rows per wave share the p chunk held in registers (four
// doubles per lane, twice k_matvec_f64's per A byte), U chunks per row are in
// flight, the loads of step c+U go out before the FMAs of step c, the grid is
// sized by occupancy and grid-strides over row groups, and the fused p.Ap goes
// through grid_sum_last_block.  A lane adds its four columns of every chunk in
// chunk order into four accumulators, then ((x + y) + (z + w)) and the wave
// sum: the same order for every (R, U, policy), so every plan gives the same
// row sums bit for bit.
#include "cgx_device.h"

#include <algorithm>

namespace cgx {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));

// A load policy: 2 default-policy loads, 8 non-temporal (both software-pipelined)
template <int NT>
__device__ __forceinline__ f4 load_a4(const f4 *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

__device__ __forceinline__ void fma4(const f4 a, const d4 p, d4 &acc) {
    acc.x = __builtin_fma((double)a.x, p.x, acc.x);
    acc.y = __builtin_fma((double)a.y, p.y, acc.y);
    acc.z = __builtin_fma((double)a.z, p.z, acc.z);
    acc.w = __builtin_fma((double)a.w, p.w, acc.w);
}

template <int R, int U, int NT>
__device__ __forceinline__ void a32_load_step(const f4 *const (&arow)[R], const d4 *v4, int64_t c, d4 (&pv)[U],
                                              f4 (&av)[R][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) pv[u] = v4[(c + u) * 64];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) av[r][u] = load_a4<NT>(arow[r] + (c + u) * 64);
}

template <int R, int U>
__device__ __forceinline__ void a32_fma_step(const d4 (&pv)[U], const f4 (&av)[R][U], d4 (&acc)[R]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) fma4(av[r][u], pv[u], acc[r]);
}

// 256-column chunks [0, nchunk) of R rows into acc: two register sets,
// ping-pong, so a wave always has a step's loads in flight.
template <int R, int U, int NT>
__device__ __forceinline__ void a32_chunks_pipe(const f4 *const (&arow)[R], const d4 *v4, int64_t nchunk,
                                                d4 (&acc)[R]) {
    d4 pa[U], pb[U];
    f4 aa[R][U], ab[R][U];
    int64_t c = 0;
    if (c + U <= nchunk) a32_load_step<R, U, NT>(arow, v4, c, pa, aa);
    while (c + U <= nchunk) {
        const bool more = c + 2 * U <= nchunk;
        if (more) a32_load_step<R, U, NT>(arow, v4, c + U, pb, ab);
        a32_fma_step<R, U>(pa, aa, acc);
        c += U;
        if (!more) break;
        const bool more2 = c + 2 * U <= nchunk;
        if (more2) a32_load_step<R, U, NT>(arow, v4, c + U, pa, aa);
        a32_fma_step<R, U>(pb, ab, acc);
        c += U;
        if (!more2) break;
    }
    for (; c < nchunk; ++c) {  // remaining single chunks
        const d4 pv = v4[c * 64];
#pragma unroll
        for (int r = 0; r < R; ++r) fma4(load_a4<NT>(arow[r] + c * 64), pv, acc[r]);
    }
}

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
    const int wid = threadIdx.x >> 6;
    const int64_t ngroups = (rows + R - 1) / R;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    const int64_t nchunk = vec_cols >> 8;
    const d4 *v4 = reinterpret_cast<const d4 *>(v) + lane;
    double dacc = 0.0;

    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t r0 = g * R;
        int64_t ridx[R];
        const f4 *arow[R];
        d4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ridx[r] = (r0 + r < rows) ? (r0 + r) : (rows - 1);
            arow[r] = reinterpret_cast<const f4 *>(A + ridx[r] * lda) + lane;
            acc[r] = (d4)(0.0);
        }
        a32_chunks_pipe<R, U, NT>(arow, v4, nchunk, acc);
        for (int64_t j = vec_cols + lane; j < cols; j += 64) {
            const double vj = v[j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r].x = __builtin_fma((double)A[ridx[r] * lda + j], vj, acc[r].x);
        }
        double mine = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double s = wave_sum((acc[r].x + acc[r].y) + (acc[r].z + acc[r].w));
            if (lane == r) mine = s;
        }
        if (lane < R && r0 + lane < rows) {
            out[r0 + lane] = mine;
            if (pown) dacc += pown[r0 + lane] * mine;
        }
    }
    if (pown) grid_sum_last_block(dacc, partials, ticket, dot_out);
    ts_end(ts);
}

using A32Fn = decltype(&k_matvec_a32<4, 4, 1>);

// The instantiated plans (cgx_set_matvec_plan accepts exactly these): rows per
// wave x 256-column chunks in flight, each with both load policies.
constexpr struct { int R, U; } kA32Plans[] = {{1, 4}, {1, 8}, {2, 4}, {4, 2}, {4, 4}, {8, 2}};

template <int NT>
A32Fn pick_a32_nt(int R, int U) {
    if (R == 1) return U == 8 ? k_matvec_a32<1, 8, NT> : k_matvec_a32<1, 4, NT>;
    if (R == 2) return k_matvec_a32<2, 4, NT>;
    if (R == 4) return U == 2 ? k_matvec_a32<4, 2, NT> : k_matvec_a32<4, 4, NT>;
    return k_matvec_a32<8, 2, NT>;
}
A32Fn pick_a32(int R, int U, int nt) { return nt == 8 ? pick_a32_nt<1>(R, U) : pick_a32_nt<0>(R, U); }

}  // namespace

bool matvec_a32_plan_ok(int R, int U, int nt) {
    if (nt != 2 && nt != 8) return false;
    for (const auto &p : kA32Plans)
        if (p.R == R && p.U == U) return true;
    return false;
}

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
    {  // CGX_MV_A32_PLAN="R=..,U=..,nt=..,bpc=..": taken when it names an instantiated plan
        const int eR = env_opt("CGX_MV_A32_PLAN", "R", pl.R), eU = env_opt("CGX_MV_A32_PLAN", "U", pl.U),
                  en = env_opt("CGX_MV_A32_PLAN", "nt", pl.nt);
        if (matvec_a32_plan_ok(eR, eU, en)) pl.R = eR, pl.U = eU, pl.nt = en;
    }
    if (R > 0) pl.R = R;
    if (U > 0) pl.U = U;
    if (nt >= 0) pl.nt = nt;
    if (!matvec_a32_plan_ok(pl.R, pl.U, pl.nt)) pl.R = 4, pl.U = 4, pl.nt = 8;
    int per_cu = 0;
    const void *fn = reinterpret_cast<const void *>(pick_a32(pl.R, pl.U, pl.nt));
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kNT, 0) != hipSuccess || per_cu <= 0) per_cu = 2;
    per_cu = env_opt("CGX_MV_A32_PLAN", "bpc", per_cu);
    if (blocks_per_cu > 0) per_cu = blocks_per_cu;
    const int64_t groups = (rows + pl.R - 1) / pl.R;
    const int64_t need = (groups + (kNT / 64) - 1) / (kNT / 64);
    int64_t cap = (int64_t)per_cu * cus;
    if (cap > kMaxRedBlocks) cap = kMaxRedBlocks;
    pl.blocks = (int)std::max<int64_t>(1, std::min(need, cap));
    return pl;
}

hipError_t matvec_a32(const MatvecPlan &pl, const float *A, int64_t lda, int64_t rows, int64_t cols, const double *v,
                      double *out, const double *pown, double *dot_out, const RedWs &ws, hipStream_t s,
                      const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    if (!pl.a32 || !matvec_a32_plan_ok(pl.R, pl.U, pl.nt) || pl.blocks < 1) return hipErrorInvalidValue;
    // The vector path needs 16-B-aligned rows and a 32-B-aligned p (a lane
    // reads four doubles); otherwise every column goes through the scalar tail.
    const bool aligned = (reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(v) & 31) == 0 &&
                         (lda & 3) == 0;
    const int64_t vec_cols = aligned ? (cols & ~int64_t(255)) : 0;
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
