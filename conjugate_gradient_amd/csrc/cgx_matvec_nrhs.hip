// cgx_matvec_nrhs.hip -- several right-hand sides per pass over A
// (cgx_create_nrhs): the dense fp64 matVec of K vectors at once, and the
// K-column vector kernels of the batched CG iteration.
//
// The dense CG iteration is the HBM-bound read of A.  K independent systems
// on one matrix (the reference: one run per vectorb.txt) share that read:
// k_matvec_nrhs_f64 loads every element of A once and multiplies it by K
// vector elements, Out_j = A V_j for j < K.  Batched CG, not block CG: the K
// recurrences share nothing but the read of A, each with its own alpha, beta
// and stopping point.
//
// Layout of the K vectors: K separate arrays, column j at V + j*ldv (Out: ldo,
// pown: ldp), not interleaved by element -- a lane's 16-B load then takes two
// consecutive elements of one vector, as k_matvec_f64's, the vector kernels
// and the host copies work on plain contiguous vectors, and a column is what
// cgx_matvec takes.  (The interleaved layout has not been measured.)
//
// The structure cgx_matvec_core.h describes, with K vectors of d2 chunks held
// in registers beside the R rows; gate and ts as k_matvec_f64's, and the K
// fused dots pown_j . out_j through one last-block hand-off
// (grid_sum_last_block_n: own partial slots and result slot per column).
//
// Summation order (a contract): every column j is summed in the non-rotated
// k_matvec_f64's order, for every instantiated (K, R, U, policy).  Row sums
// are therefore the bits of cgx_matvec(CGX_F64) on that column alone under
// every plan.
//
// Registers per lane (32-bit VGPRs): accumulators 4 R K, one A set 4 R U, one
// vector set 4 K U, two sets in the pipeline; 256 threads per block, one wave
// per SIMD, so up to 512 (VGPR + AGPR).  No instantiated plan uses scratch
// (DESIGN.md lists every instantiation's resource usage).
#include "cgx_matvec_core.h"

#include <algorithm>
#include <iterator>

namespace cgx {
namespace {

// k_matvec_nrhs_f64 keeps its own load / FMA steps, pipeline, walk and epilogue
// (cgx_matvec_core.h's structure; only the A load policy is shared): built from
// the shared pieces the K = 8 default at 65536^2, <8, 4, 1>, measured 1.2 %
// slower per iteration (6.888 against 6.806 ms, profiles/matvec_core_ab.jsonl).
template <int K, int R, int U, int NT>
__device__ __forceinline__ void nr_load_step(const d2 *const (&arow)[R], const d2 *const (&v2)[K], int64_t c,
                                             d2 (&pv)[K][U], d2 (&av)[R][U]) {
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) pv[j][u] = v2[j][(c + u) * 64];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) av[r][u] = load_a<NT>(arow[r] + (c + u) * 64);
}

template <int K, int R, int U>
__device__ __forceinline__ void nr_fma_step(const d2 (&pv)[K][U], const d2 (&av)[R][U], d2 (&acc)[K][R]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                acc[j][r].x = __builtin_fma(av[r][u].x, pv[j][u].x, acc[j][r].x);
                acc[j][r].y = __builtin_fma(av[r][u].y, pv[j][u].y, acc[j][r].y);
            }
}

// 128-column chunks [0, nchunk) of R rows against K vectors: two register sets, ping-pong.
template <int K, int R, int U, int NT>
__device__ __forceinline__ void nr_chunks_pipe(const d2 *const (&arow)[R], const d2 *const (&v2)[K], int64_t nchunk,
                                               d2 (&acc)[K][R]) {
    d2 pa[K][U], pb[K][U], aa[R][U], ab[R][U];
    int64_t c = 0;
    if (c + U <= nchunk) nr_load_step<K, R, U, NT>(arow, v2, c, pa, aa);
    while (c + U <= nchunk) {
        const bool more = c + 2 * U <= nchunk;
        if (more) nr_load_step<K, R, U, NT>(arow, v2, c + U, pb, ab);
        nr_fma_step<K, R, U>(pa, aa, acc);
        c += U;
        if (!more) break;
        const bool more2 = c + 2 * U <= nchunk;
        if (more2) nr_load_step<K, R, U, NT>(arow, v2, c + U, pa, aa);
        nr_fma_step<K, R, U>(pb, ab, acc);
        c += U;
        if (!more2) break;
    }
    for (; c < nchunk; ++c) {  // remaining single chunks
        d2 pv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) pv[j] = v2[j][c * 64];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const d2 a = load_a<NT>(arow[r] + c * 64);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                acc[j][r].x = __builtin_fma(a.x, pv[j].x, acc[j][r].x);
                acc[j][r].y = __builtin_fma(a.y, pv[j].y, acc[j][r].y);
            }
        }
    }
}

// vec_cols (a multiple of 128; 0 when a pointer or a pitch is not 16-B
// aligned) columns go through the vector path, [vec_cols, cols) through the
// scalar tail.  Columns nrhs..K-1 read column 0 again and store nothing.
template <int K, int R, int U, int NT>
__global__ __launch_bounds__(kNT) void k_matvec_nrhs_f64(
    const double *__restrict__ A, int64_t lda, int64_t rows, int64_t cols, int64_t vec_cols, int nrhs,
    const double *__restrict__ V, int64_t ldv, double *__restrict__ Out, int64_t ldo,
    const double *__restrict__ pown, int64_t ldp, double *dot_out, double *partials, unsigned *ticket,
    const int64_t *gate, int64_t *ts) {
    if (gate && *gate) return;  // every column stopped in an earlier iteration (device-side gating)
    ts_start(ts);
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int64_t ngroups = (rows + R - 1) / R;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    const int64_t nchunk = vec_cols >> 7;
    const double *vj[K];
    const d2 *v2[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        vj[j] = V + (j < nrhs ? j : 0) * ldv;
        v2[j] = reinterpret_cast<const d2 *>(vj[j]) + lane;
    }
    double dacc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) dacc[j] = 0.0;

    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t r0 = g * R;
        int64_t ridx[R];
        const d2 *arow[R];
        d2 acc[K][R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ridx[r] = (r0 + r < rows) ? (r0 + r) : (rows - 1);
            arow[r] = reinterpret_cast<const d2 *>(A + ridx[r] * lda) + lane;
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j][r] = (d2)(0.0);
        }
        nr_chunks_pipe<K, R, U, NT>(arow, v2, nchunk, acc);
        for (int64_t c = vec_cols + lane; c < cols; c += 64) {
            double vc[K];
#pragma unroll
            for (int j = 0; j < K; ++j) vc[j] = vj[j][c];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double a = A[ridx[r] * lda + c];
#pragma unroll
                for (int j = 0; j < K; ++j) acc[j][r].x = __builtin_fma(a, vc[j], acc[j][r].x);
            }
        }
        double mine[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            mine[j] = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double s = wave_sum(acc[j][r].x + acc[j][r].y);
                if (lane == r) mine[j] = s;
            }
        }
        if (lane < R && r0 + lane < rows) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < nrhs) {
                    Out[j * ldo + r0 + lane] = mine[j];
                    if (pown) dacc[j] += pown[j * ldp + r0 + lane] * mine[j];
                }
        }
    }
    if (pown) grid_sum_last_block_n<K>(dacc, partials, ticket, dot_out, (1u << nrhs) - 1u);
    ts_end(ts);
}

using NrFn = decltype(&k_matvec_nrhs_f64<2, 4, 4, 1>);

// The instantiated plans per K (cgx_set_matvec_plan accepts exactly these):
// rows per wave x 128-column chunks in flight, each with both load policies.
struct NrPlan {
    int K, R, U;
};
constexpr NrPlan kNrPlans[] = {{2, 2, 4}, {2, 4, 2}, {2, 4, 4}, {2, 8, 2},  //
                               {4, 4, 2}, {4, 4, 4}, {4, 8, 2},             //
                               {8, 4, 1}, {8, 4, 2}};
// (K = 8 with eight rows per wave needs 256 accumulator registers and two
// register sets beside them: R = 8, U = 1 compiles to 216 bytes of scratch per
// lane, so it is not instantiated.)

// the listed plan's kernel, or nullptr
template <int NT, size_t I = 0>
NrFn pick_nrhs_nt(int K, int R, int U) {
    if constexpr (I == std::size(kNrPlans)) return nullptr;
    else {
        constexpr NrPlan p = kNrPlans[I];
        return (p.K == K && p.R == R && p.U == U) ? k_matvec_nrhs_f64<p.K, p.R, p.U, NT>
                                                  : pick_nrhs_nt<NT, I + 1>(K, R, U);
    }
}
NrFn pick_nrhs(int K, int R, int U, int nt) {
    return nt == 8 ? pick_nrhs_nt<1>(K, R, U) : nt == 2 ? pick_nrhs_nt<0>(K, R, U) : nullptr;
}

// ---------------------------------------------------------------------------
// The K-column vector kernels (serialConjugate.c:209-243 per column).  A
// thread owns element pairs; the last odd element of a column goes alone.
// Per-thread sums in a fixed order, then the deterministic grid reduction, so
// a column's scalars do not depend on the other columns.
// ---------------------------------------------------------------------------
#define CGX_NRHS_PAIR_LOOP(q) \
    for (int64_t q = (int64_t)blockIdx.x * kNT + threadIdx.x; 2 * q < n; q += (int64_t)gridDim.x * kNT)

template <int K>
__global__ __launch_bounds__(kNT) void k_nrhs_residual_f64(int64_t n, int64_t ld, int nrhs,
                                                           const double *__restrict__ b,
                                                           const double *__restrict__ Ax, double *__restrict__ r,
                                                           double *__restrict__ p, double *out, NrhsScal *clear,
                                                           int64_t *hrec, double *partials, unsigned *ticket) {
    if (clear && blockIdx.x == 0 && threadIdx.x < kMaxNrhs) {
        clear->kdone[threadIdx.x] = 0;
        clear->rrfinal[threadIdx.x] = 0.0;
        if (threadIdx.x == 0) {
            clear->alldone = 0;
            if (hrec) __hip_atomic_store(hrec, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        acc[j] = 0.0;
        if (j >= nrhs) continue;
        const int64_t o = j * ld;
        CGX_NRHS_PAIR_LOOP(q) {
            const int64_t i = 2 * q;
            if (i + 1 < n) {
                const d2 ri = ld2(b + o + i) - (Ax ? ld2(Ax + o + i) : (d2)(0.0));
                st2(r + o + i, ri);
                if (p) st2(p + o + i, ri);
                acc[j] += ri.x * ri.x + ri.y * ri.y;
            } else {
                const double ri = b[o + i] - (Ax ? Ax[o + i] : 0.0);
                r[o + i] = ri;
                if (p) p[o + i] = ri;
                acc[j] += ri * ri;
            }
        }
    }
    grid_sum_last_block_n<K>(acc, partials, ticket, out, (1u << nrhs) - 1u);
}

template <int K>
__global__ __launch_bounds__(kNT) void k_nrhs_dot_f64(int64_t n, int64_t ld, int nrhs, const double *__restrict__ a,
                                                      const double *__restrict__ b, double *out, double *partials,
                                                      unsigned *ticket) {
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        acc[j] = 0.0;
        if (j >= nrhs) continue;
        const int64_t o = j * ld;
        CGX_NRHS_PAIR_LOOP(q) {
            const int64_t i = 2 * q;
            if (i + 1 < n) {
                const d2 av = ld2(a + o + i), bv = ld2(b + o + i);
                acc[j] += av.x * bv.x + av.y * bv.y;
            } else {
                acc[j] += a[o + i] * b[o + i];
            }
        }
    }
    grid_sum_last_block_n<K>(acc, partials, ticket, out, (1u << nrhs) - 1u);
}

// r_j -= alpha_j Ap_j; r_j.r_j.  This launch precedes the iteration's stopping
// decision, so a non-zero kdone[j] or alldone was stored by an earlier
// iteration: that column (every column) is frozen.
template <int K>
__global__ __launch_bounds__(kNT) void k_nrhs_update_r_f64(int64_t n, int64_t ld, int nrhs, int ring_k, int ring_k1,
                                                           double *__restrict__ r, const double *__restrict__ Ap,
                                                           NrhsScal *sc, double *partials, unsigned *ticket) {
    if (sc->alldone) return;
    double acc[K];
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        acc[j] = 0.0;
        if (j >= nrhs || sc->kdone[j] != 0) continue;
        mask |= 1u << j;
        const double alpha = cg_ratio(sc->rr[ring_k][j], sc->pap[ring_k][j]);
        const int64_t o = j * ld;
        CGX_NRHS_PAIR_LOOP(q) {
            const int64_t i = 2 * q;
            if (i + 1 < n) {
                const d2 ri = ld2(r + o + i) - alpha * ld2(Ap + o + i);
                st2(r + o + i, ri);
                acc[j] += ri.x * ri.x + ri.y * ri.y;
            } else {
                const double ri = r[o + i] - alpha * Ap[o + i];
                r[o + i] = ri;
                acc[j] += ri * ri;
            }
        }
    }
    grid_sum_last_block_n<K>(acc, partials, ticket, sc->rr[ring_k1], mask);
}

// x_j += alpha_j p_j, then the reference's stopping decision per column
// (serialConjugate.c:235-238: sqrt(r.r) < EPSILON breaks before the p update)
// or p_j = r_j + beta_j p_j.  Block 0's first thread records the decisions;
// the records it stores hold k+1, which no block of this launch takes for
// "frozen" (kdone in (0, k]), so every block decides alike.
template <int K>
__global__ __launch_bounds__(kNT) void k_nrhs_update_xp_f64(int64_t n, int64_t ld, int nrhs, int64_t k, int ring_k,
                                                            int ring_k1, double eps, double *__restrict__ x,
                                                            double *__restrict__ p, const double *__restrict__ r,
                                                            NrhsScal *sc, int64_t *hrec) {
    const int64_t ad = sc->alldone;
    if (ad != 0 && ad <= k) return;
    int ndone = 0, nnew = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j >= nrhs) continue;
        const int64_t kd = sc->kdone[j];
        if (kd != 0 && kd <= k) {
            ++ndone;
            continue;
        }
        const double rrn = sc->rr[ring_k1][j], rso = sc->rr[ring_k][j];
        const bool stop = eps >= 0.0 && sqrt(rrn) < eps;
        const double alpha = cg_ratio(rso, sc->pap[ring_k][j]);
        const double beta = stop ? 0.0 : cg_ratio(rrn, rso);
        if (stop) {
            ++ndone;
            ++nnew;
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                sc->rrfinal[j] = rrn;
                sc->kdone[j] = k + 1;
            }
        }
        const int64_t o = j * ld;
        CGX_NRHS_PAIR_LOOP(q) {
            const int64_t i = 2 * q;
            if (i + 1 < n) {
                const d2 pv = ld2(p + o + i);
                st2(x + o + i, ld2(x + o + i) + alpha * pv);
                if (!stop) st2(p + o + i, ld2(r + o + i) + beta * pv);
            } else {
                const double pv = p[o + i];
                x[o + i] = x[o + i] + alpha * pv;
                if (!stop) p[o + i] = r[o + i] + beta * pv;
            }
        }
    }
    if (nnew > 0 && ndone == nrhs && blockIdx.x == 0 && threadIdx.x == 0) {
        sc->alldone = k + 1;
        if (hrec) __hip_atomic_store(hrec, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <class F2, class F4, class F8>
auto pick_k(int nrhs, F2 f2, F4 f4, F8 f8) {
    const int K = nrhs_width(nrhs);
    return K == 2 ? f2 : K == 4 ? f4 : f8;
}

}  // namespace

bool matvec_nrhs_plan_ok(int K, int R, int U, int nt) { return pick_nrhs(K, R, U, nt) != nullptr; }

MatvecPlan plan_matvec_nrhs(int device, int64_t rows, int K, int R, int U, int nt, int blocks_per_cu, int64_t cols) {
    MatvecPlan pl;
    pl.nrhs = K;
    const int cus = cu_count(device);
    // Measured on MI355X, every instantiated plan of a width interleaved with
    // the k_matvec_f64 default in the same rounds (profiles/nrhs_sweep_k{2,4,8}_n*.jsonl,
    // median ms per launch, non-temporal loads; default-policy loads are 9-15 %
    // slower at these sizes).  What sets the rate is the ratio of vector bytes
    // to A bytes per chunk, K / R, as the float-A sweep found
    // (profiles/a32_sweep_plans_n65536.jsonl).
    //   K = 2: R = 4, U = 4 at both sizes -- 4.866 ms at 65536^2 against 4.859
    //     for k_matvec_f64 (8,2: 4.950; 4,2: 4.959; 2,4: 5.354), 0.3245 against
    //     0.3171 at 16384^2 (4,2 and 8,2: 0.3410).
    //   K = 4: R = 8, U = 2 at both sizes -- 4.957 against 4.860 at 65536^2
    //     (4,4: 5.341; 4,2: 5.529), 0.3269 against 0.3147 at 16384^2 (4,4:
    //     0.3493), where a resident wave has two row groups; below that it is
    //     not measured and four rows per wave are kept.
    //   K = 8: four rows per wave at most (eight need scratch), ratio 2, and the
    //     stream falls to 5.0 TB/s on A: R = 4, U = 1 6.789 ms at 65536^2 (U = 2:
    //     6.904) against 4.867, U = 2 0.4444 at 16384^2 (U = 1: 0.4504) against
    //     0.3152.  Eight systems still cost 1.43 passes of one; staging the
    //     vectors in LDS is the form left to try.
    const int64_t want_waves = (int64_t)cus * 4;
    if (K == 2) pl.R = 4, pl.U = 4;
    else if (K == 4) pl.R = rows >= 16 * want_waves ? 8 : 4, pl.U = pl.R == 8 ? 2 : 4;
    else pl.R = 4, pl.U = rows >= 32 * want_waves ? 1 : 2;
    // an A of up to 64 MiB with default-policy loads, so it stays in the MALL
    // between iterations (as plan_matvec_f64)
    pl.nt = (cols > 0 && rows * cols * 8 <= (int64_t(64) << 20)) ? 2 : 8;
    // CGX_MV_NRHS_PLAN="R=..,U=..,nt=..,bpc=..": taken when it names an instantiated plan;
    // the fallback R = 4, U = 2 is instantiated for every K
    plan_listed(pl, "CGX_MV_NRHS_PLAN", R, U, nt, matvec_nrhs_plan_ok, 4, 2);
    pl.blocks = plan_grid(reinterpret_cast<const void *>(pick_nrhs(K, pl.R, pl.U, pl.nt)), device, rows, pl.R, 1,
                          "CGX_MV_NRHS_PLAN", blocks_per_cu);
    return pl;
}

hipError_t matvec_nrhs_f64(const MatvecPlan &pl, const double *A, int64_t lda, int64_t rows, int64_t cols, int nrhs,
                           const double *V, int64_t ldv, double *Out, int64_t ldo, const double *pown, int64_t ldp,
                           double *dot_out, const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    if (nrhs < 1 || nrhs > kMaxNrhs || pl.nrhs != nrhs_width(nrhs) || !matvec_nrhs_plan_ok(pl.nrhs, pl.R, pl.U, pl.nt) ||
        pl.blocks < 1 || pl.blocks > kMaxRedBlocks)
        return hipErrorInvalidValue;
    // The vector path needs 16-B-aligned rows and vectors (every column: an
    // even ldv when there is more than one); otherwise every column of A goes
    // through the scalar tail, as matvec_f64 decides for one vector.
    const int64_t vec_cols =
        matvec_vec_cols((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(V)) & 15,
                        (lda & 1) == 0 && (nrhs == 1 || (ldv & 1) == 0), cols, 128);
    hipLaunchKernelGGL(pick_nrhs(pl.nrhs, pl.R, pl.U, pl.nt), dim3(pl.blocks), dim3(kNT), 0, s, A, lda, rows, cols,
                       vec_cols, nrhs, V, ldv, Out, ldo, pown, ldp, dot_out, ws.partials, ws.tickets + TN_MATVEC, gate,
                       ts);
    return hipGetLastError();
}

static bool nrhs_vec_ok(int64_t n, int64_t ld, int nrhs, std::initializer_list<const void *> ptrs) {
    if (n < 1 || nrhs < 1 || nrhs > kMaxNrhs || ld < n || (ld & 1)) return false;
    for (const void *p : ptrs)
        if (p && !al16(p)) return false;
    return true;
}

hipError_t nrhs_residual_f64(int64_t n, int64_t ld, int nrhs, const double *b, const double *Ax, double *r, double *p,
                             double *out, NrhsScal *clear, int64_t *hrec, const RedWs &ws, hipStream_t s) {
    if (!nrhs_vec_ok(n, ld, nrhs, {b, Ax, r, p})) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pick_k(nrhs, k_nrhs_residual_f64<2>, k_nrhs_residual_f64<4>, k_nrhs_residual_f64<8>),
                       dim3(grid_vec(n)), dim3(kNT), 0, s, n, ld, nrhs, b, Ax, r, p, out, clear, hrec, ws.partials,
                       ws.tickets + TN_RESID);
    return hipGetLastError();
}

hipError_t nrhs_dot_f64(int64_t n, int64_t ld, int nrhs, const double *a, const double *b, double *out,
                        const RedWs &ws, hipStream_t s) {
    if (!nrhs_vec_ok(n, ld, nrhs, {a, b})) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pick_k(nrhs, k_nrhs_dot_f64<2>, k_nrhs_dot_f64<4>, k_nrhs_dot_f64<8>), dim3(grid_vec(n)),
                       dim3(kNT), 0, s, n, ld, nrhs, a, b, out, ws.partials, ws.tickets + TN_DOT);
    return hipGetLastError();
}

hipError_t nrhs_update_r_f64(int64_t n, int64_t ld, int nrhs, int64_t k, double *r, const double *Ap, NrhsScal *sc,
                             const RedWs &ws, hipStream_t s) {
    if (!nrhs_vec_ok(n, ld, nrhs, {r, Ap})) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pick_k(nrhs, k_nrhs_update_r_f64<2>, k_nrhs_update_r_f64<4>, k_nrhs_update_r_f64<8>),
                       dim3(grid_vec(n)), dim3(kNT), 0, s, n, ld, nrhs, (int)(k & 3), (int)((k + 1) & 3), r, Ap, sc,
                       ws.partials, ws.tickets + TN_R);
    return hipGetLastError();
}

hipError_t nrhs_update_xp_f64(int64_t n, int64_t ld, int nrhs, int64_t k, double eps, double *x, double *p,
                              const double *r, NrhsScal *sc, int64_t *hrec, hipStream_t s) {
    if (!nrhs_vec_ok(n, ld, nrhs, {x, p, r})) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pick_k(nrhs, k_nrhs_update_xp_f64<2>, k_nrhs_update_xp_f64<4>, k_nrhs_update_xp_f64<8>),
                       dim3(grid_vec(n)), dim3(kNT), 0, s, n, ld, nrhs, k, (int)(k & 3), (int)((k + 1) & 3), eps, x, p, r,
                       sc, hrec);
    return hipGetLastError();
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_matvec_nrhs() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_nrhs_dot_f64<2>));
}

}  // namespace cgx
