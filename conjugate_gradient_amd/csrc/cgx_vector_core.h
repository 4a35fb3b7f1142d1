// cgx_vector_core.h -- internal to libcgx, for the files that hold fp64
// element-wise kernels (cgx_vector.hip, cgx_pcg.hip, cgx_pcg_block.hip): the
// one element pass vec_pass, and the element expressions that more than one
// kernel uses, each spelled once for a pair (d2) and for one element (double).
//
// A kernel names its input streams and gives one generic callable
//   body(i, io, v0, v1, ...)
// with i the index of the element (the first of a pair), v_k what stream k
// holds there (0.0 where an optional stream is absent) and io the matching
// store: io.st(ptr + i, value).  decltype(io)::pair tells a body that stores
// some other way which form it is in (k_update_xrp_f64's write-through r).
//
// vec_pass<VEC, VP> owns the loops.  VEC (every pointer 16-B aligned): a block
// step covers kVU * kNT consecutive element pairs; each thread loads its kVU
// pairs of every stream (16-B loads of policy VP, all issued before the first
// body runs, so before any store), then runs the body on pair u = 0 .. kVU-1;
// the odd last element is done by thread 0 of block 0, after its pairs.
// Otherwise a scalar grid-stride loop with plain loads and stores.  The pass
// does no arithmetic: sums, their order (a thread's bodies run in ascending i,
// the odd element last) and fp contraction are the body's.  A body that needs
// contraction off says so inside its own braces (the pragma is lexical).
#pragma once

#include "cgx_device.h"

#include <utility>

namespace cgx {

// An input stream.  OPT: absent when !on -- not loaded, reads as 0.0 (only
// such a stream costs a run-time test).  VP >= 0: this stream's own load
// policy instead of the pass's.
template <bool OPT, int VP>
struct VecIn {
    const double *p;
    bool on;
};
template <int VP = -1>
__device__ __forceinline__ VecIn<false, VP> vin(const double *p) { return {p, true}; }
template <int VP = -1>
__device__ __forceinline__ VecIn<true, VP> vopt(const double *p, bool on) { return {p, on}; }

template <int VP>
struct PairIO {
    static constexpr bool pair = true;
    __device__ __forceinline__ void st(double *p, d2 v) const { stv<VP>(p, v); }
};
struct ScalarIO {
    static constexpr bool pair = false;
    __device__ __forceinline__ void st(double *p, double v) const { *p = v; }
};

template <int PVP, bool OPT, int VP>
__device__ __forceinline__ d2 vec_ld2(VecIn<OPT, VP> s, int64_t i) {
    if (OPT && !s.on) return (d2)(0.0);
    return ldv<(VP >= 0 ? VP : PVP)>(s.p + i);
}
template <bool OPT, int VP>
__device__ __forceinline__ double vec_ld1(VecIn<OPT, VP> s, int64_t i) {
    return (OPT && !s.on) ? 0.0 : s.p[i];
}
template <int PVP, size_t... K, class... S>
__device__ __forceinline__ void vec_load(d2 *v, int64_t i, std::index_sequence<K...>, S... s) {
    ((v[K] = vec_ld2<PVP>(s, i)), ...);
}
template <class F, class IO, size_t... K>
__device__ __forceinline__ void vec_body(F &body, int64_t i, IO io, const d2 *v, std::index_sequence<K...>) {
    body(i, io, v[K]...);
}

template <bool VEC, int VP, class F, class... S>
__device__ __forceinline__ void vec_pass(int64_t n, F body, S... s) {
    if constexpr (VEC) {
        constexpr std::index_sequence_for<S...> ks{};
        const int64_t npairs = n >> 1;
        const int64_t step = (int64_t)gridDim.x * kNT * kVU;
        for (int64_t base = (int64_t)blockIdx.x * kNT * kVU + threadIdx.x; base < npairs; base += step) {
            bool ok[kVU];
#pragma unroll
            for (int u = 0; u < kVU; ++u) ok[u] = base + u * kNT < npairs;
            d2 v[kVU][sizeof...(S)];
#pragma unroll
            for (int u = 0; u < kVU; ++u)
                if (ok[u]) vec_load<VP>(v[u], 2 * (base + u * kNT), ks, s...);
#pragma unroll
            for (int u = 0; u < kVU; ++u)
                if (ok[u]) vec_body(body, 2 * (base + u * kNT), PairIO<VP>{}, v[u], ks);
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) body(n - 1, ScalarIO{}, vec_ld1(s, n - 1)...);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT)
            body(i, ScalarIO{}, vec_ld1(s, i)...);
    }
}

// The plain kernels' element expressions (contraction as the file is built:
// hipcc fuses each into one FMA per element).
template <class V>
__device__ __forceinline__ V axpy_x(V x, double alpha, V p) { return x + alpha * p; }  // x += alpha p
template <class V>
__device__ __forceinline__ V sub_r(V r, double alpha, V Ap) { return r - alpha * Ap; }  // r -= alpha Ap
template <class V>
__device__ __forceinline__ V next_p(V r, double beta, V p) { return r + beta * p; }  // p = r + beta p
// what a pair, or one element, adds to a dot product
__device__ __forceinline__ double elem_dot(d2 a, d2 b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ double elem_dot(double a, double b) { return a * b; }

// The preconditioned kernels' forms of the same (contraction off, the fused
// operations spelled out: the contract at the head of cgx_pcg.hip).
__device__ __forceinline__ d2 vfma(double a, d2 b, d2 c) {
    d2 o;
    o.x = __builtin_fma(a, b.x, c.x);
    o.y = __builtin_fma(a, b.y, c.y);
    return o;
}
__device__ __forceinline__ double vfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ d2 vmul(d2 a, d2 b) {
#pragma clang fp contract(off)
    d2 o;
    o.x = a.x * b.x;
    o.y = a.y * b.y;
    return o;
}
__device__ __forceinline__ double vmul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
// acc + (a.x b.x + a.y b.y) as the plain kernels' `acc += elem_dot(a, b)` compiles for a pair,
// and fma(a, b, acc) as it compiles for the odd last element
__device__ __forceinline__ double dot_acc(double acc, d2 a, d2 b) {
#pragma clang fp contract(off)
    const double t = a.y * b.y;
    return acc + __builtin_fma(a.x, b.x, t);
}
__device__ __forceinline__ double dot_acc(double acc, double a, double b) { return __builtin_fma(a, b, acc); }

}  // namespace cgx
