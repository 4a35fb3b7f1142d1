// cgx_matvec_core.h -- internal to libcgx, device code only: the row-streaming
// skeleton k_matvec_fold_f64 (cgx_matvec.hip) and k_matvec_a32 are built from.
// k_matvec_f64 and k_matvec_nrhs_f64 have the same structure in code of their
// own, each of which measured faster than the shared form (see there); they
// share the load policy, as k_matvec_small_f64 does.
//
// Structure.  A is streamed once with 16-B-per-lane coalesced
// loads: a wave covers one 1-KiB chunk of a row per instruction -- 128 columns
// of a double A (a d2 per lane), 256 of a float A (an f4 per lane).  A wave
// owns row groups g = w, w + waves, ... of R consecutive rows, which share the
// chunks of the K vectors held in registers; a step is U chunks of every row,
// and the loads of step c+U are issued before the FMAs of step c (two register
// sets, ping-pong), so a wave always has a step's loads in flight.
//
// Summation order (a contract; tests/_matvec_order.py states it on the CPU):
// per row and vector a lane keeps one accumulator per element of its A vector
// (.x .y, or .x .y .z .w), adds element e of every chunk into accumulator e in
// chunk order with one FMA each, then the scalar tail columns into .x; then
// x + y, or (x + y) + (z + w); then the wave sum.  R, U, K and the load policy
// change which FMAs are in flight together, never a chain: every plan gives
// the same row sums bit for bit.
#pragma once
#include "cgx_device.h"

namespace cgx {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));

// Load policy of the A stream (the only data a matVec reads once): NT = 0 the
// default policy, 1 non-temporal.  The variants measured and not adopted
// (buffer loads with other cache bits, a flattened pipeline, LDS-staged p, SGPR
// row bases) live in tools/microbench/matvec_variants.hip.
template <int NT, class T>
__device__ __forceinline__ T load_a(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// One A vector times the matching vector elements, element e into accumulator e.
__device__ __forceinline__ void fma_vec(const d2 a, const d2 p, d2 &acc) {
    acc.x = __builtin_fma(a.x, p.x, acc.x);
    acc.y = __builtin_fma(a.y, p.y, acc.y);
}
__device__ __forceinline__ void fma_vec(const f4 a, const d4 p, d4 &acc) {  // v_cvt_f64_f32 is exact
    acc.x = __builtin_fma((double)a.x, p.x, acc.x);
    acc.y = __builtin_fma((double)a.y, p.y, acc.y);
    acc.z = __builtin_fma((double)a.z, p.z, acc.z);
    acc.w = __builtin_fma((double)a.w, p.w, acc.w);
}
__device__ __forceinline__ double lane_sum(const d2 a) { return a.x + a.y; }
__device__ __forceinline__ double lane_sum(const d4 a) { return (a.x + a.y) + (a.z + a.w); }

// The vector operand of a matVec: load(c) is what a lane fetches of chunk c
// (issued a step ahead), get() turns it into the multiplier at the FMA step,
// at(j) is element j for the scalar tail.  VecPlain: the vector as stored (PV =
// d2 beside a d2 A, d4 beside an f4 A).  `v` is the vector at this lane.
template <class PV>
struct VecPlain {
    using Raw = PV;
    const double *s;
    const PV *v;
    __device__ __forceinline__ Raw load(int64_t c) const { return v[c * 64]; }
    __device__ __forceinline__ PV get(const Raw &x) const { return x; }
    __device__ __forceinline__ double at(int64_t j) const { return s[j]; }
};
template <class PV>
__device__ __forceinline__ VecPlain<PV> vec_plain(const double *v, int lane) {
    return {v, reinterpret_cast<const PV *>(v) + lane};
}

// Load step / FMA step of U chunks from chunk c: R rows of A, K vectors.  The
// FMA nesting (u outer, then r, then the vector) and the per-element chains
// are the order contract: they stay exactly as they are.
template <int NT, class AV, class P, int K, int R, int U>
__device__ __forceinline__ void load_step(const AV *const (&arow)[R], const P (&vec)[K], int64_t c,
                                          typename P::Raw (&pv)[K][U], AV (&av)[R][U]) {
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) pv[j][u] = vec[j].load(c + u);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) av[r][u] = load_a<NT>(arow[r] + (c + u) * 64);
}

template <class AV, class P, class Acc, int K, int R, int U>
__device__ __forceinline__ void fma_step(const P (&vec)[K], const typename P::Raw (&pv)[K][U], const AV (&av)[R][U],
                                         Acc (&acc)[K][R]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        decltype(vec[0].get(pv[0][u])) p[K];  // the multipliers: the operand's type, not the accumulator's
#pragma unroll
        for (int j = 0; j < K; ++j) p[j] = vec[j].get(pv[j][u]);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) fma_vec(av[r][u], p[j], acc[j][r]);
    }
}

// Chunks [c0, c1) one at a time: the remainder of a range that is no multiple of U.
template <int NT, class AV, class P, class Acc, int K, int R>
__device__ __forceinline__ void chunks_single(const AV *const (&arow)[R], const P (&vec)[K], int64_t c0, int64_t c1,
                                              Acc (&acc)[K][R]) {
    for (int64_t c = c0; c < c1; ++c) {
        typename P::Raw pv[K][1];
        AV av[R][1];
        load_step<NT>(arow, vec, c, pv, av);
        fma_step(vec, pv, av, acc);
    }
}

// The software pipeline over chunks [c0, c1): steps of U chunks with two
// register sets, the next step's loads issued before this step's FMAs, then
// the remaining single chunks.
template <int NT, int U, class AV, class P, class Acc, int K, int R>
__device__ __forceinline__ void chunks_pipe(const AV *const (&arow)[R], const P (&vec)[K], int64_t c0, int64_t c1,
                                            Acc (&acc)[K][R]) {
    typename P::Raw pa[K][U], pb[K][U];
    AV aa[R][U], ab[R][U];
    int64_t c = c0;
    if (c + U <= c1) load_step<NT>(arow, vec, c, pa, aa);
    while (c + U <= c1) {
        const bool more = c + 2 * U <= c1;
        if (more) load_step<NT>(arow, vec, c + U, pb, ab);
        fma_step(vec, pa, aa, acc);
        c += U;
        if (!more) break;
        const bool more2 = c + 2 * U <= c1;
        if (more2) load_step<NT>(arow, vec, c + U, pa, aa);
        fma_step(vec, pb, ab, acc);
        c += U;
        if (!more2) break;
    }
    chunks_single<NT>(arow, vec, c, c1, acc);
}

// Scalar tail: columns [c0, cols) (past the last whole chunk, or every column
// when a pointer or the pitch is off the 16-B grid), 64 per trip, into .x.
template <class T, class P, class Acc, int K, int R>
__device__ __forceinline__ void tail_cols(const T *A, int64_t lda, const int64_t (&ridx)[R], const P (&vec)[K],
                                          int lane, int64_t c0, int64_t cols, Acc (&acc)[K][R]) {
    for (int64_t c = c0 + lane; c < cols; c += 64) {
        double vc[K];
#pragma unroll
        for (int j = 0; j < K; ++j) vc[j] = vec[j].at(c);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double a = (double)A[ridx[r] * lda + c];
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j][r].x = __builtin_fma(a, vc[j], acc[j][r].x);
        }
    }
}

// The wave's walk over its row groups: body(r0, ridx, arow, acc) per group of
// R rows from r0 -- ridx the row indices (rows past the end clamped to the
// last row: loaded again, never stored), arow the rows at this lane, acc the
// K x R zeroed accumulators.
template <int K, int R, class AV, class Acc, class T, class F>
__device__ __forceinline__ void for_row_groups(const T *A, int64_t lda, int64_t rows, F body) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int64_t ngroups = (rows + R - 1) / R;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t r0 = g * R;
        int64_t ridx[R];
        const AV *arow[R];
        Acc acc[K][R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ridx[r] = (r0 + r < rows) ? (r0 + r) : (rows - 1);
            arow[r] = reinterpret_cast<const AV *>(A + ridx[r] * lda) + lane;
#pragma unroll
            for (int j = 0; j < K; ++j) acc[j][r] = (Acc)(0.0);
        }
        body(r0, ridx, arow, acc);
    }
}

// Row-sum epilogue: per row the wave sum of the lanes' component sums; lane r
// keeps row r's (the other lanes 0) and, when that row exists, stores it.
template <class Acc, int R>
__device__ __forceinline__ double row_sums(const Acc (&acc)[R], int lane) {
    double mine = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double s = wave_sum(lane_sum(acc[r]));
        if (lane == r) mine = s;
    }
    return mine;
}
// out[i] = mine and the fused-dot term pown[i] * mine
__device__ __forceinline__ void store_row(int64_t i, double mine, double *out, const double *pown, double &dacc) {
    out[i] = mine;
    if (pown) dacc += pown[i] * mine;
}

}  // namespace cgx
