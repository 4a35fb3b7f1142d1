// cgx_dia_core.h -- internal to libcgx: what the two diagonal-storage matVecs
// share, k_dia_mult_f64 (cgx_dia.hip, every diagonal stored) and
// k_dia_sym_mult_f64 (cgx_dia_sym.hip, the upper diagonals of a symmetric A).
// Both kernels are one walk, dia_walk, over two term policies; both files keep a
// code object, a plan rule and an order contract of their own.
//
// The walk.  One row per lane (R = 1) or two (R = 2, rows (i, i + 1) with i
// even): a wave owns 64 R consecutive rows, waves take these groups with a grid
// stride as for_row_groups does (cgx_matvec_core.h).  The offsets are
// wave-uniform (scalar loads); every wave reads them once for omin =
// min(0, min o) and omax = max(0, max o).  A group the policy calls interior
// (every term of every diagonal reaches every one of its rows) runs with no
// test at all, U diagonals per trip, their loads issued before their FMAs, then
// the ndiag % U left over one at a time.  Every other group (the first and last
// rows, a partial last group) runs one row at a time through the policy's
// guarded form: indices clamped into the arrays, loaded, the term selected away
// before the FMA, so there is no branch around a load.  Which path a row takes
// does not change its bits: one accumulator per row from +0.0, the terms in the
// policy's order, no cross-lane combine.
//
// With R = 2 two consecutive doubles at an even index are one 16-byte load
// (load_piece).  The host side sees to an even pitch and 16-byte aligned bases
// and passes vec = 0 where a kernel-level caller's arrays are not: then every
// load is 8 bytes, the bits the same.
//
// The fused p.Ap goes through store_row / grid_sum_last_block_n<1> as in the CSR
// kernel: deterministic for a given (R, grid).  No atomics, no spin-waits in the
// walk: plain vector loads and stores (the reduction hand-off is cgx_device.h's).
//
// A term policy `Terms` has three members, all __forceinline__:
//   interior<R, U, NT>(offsets, data, ld, v, i0, k0, vec, acc)   U diagonals from k0, rows i0 .. i0 + R - 1
//   guarded<U, NT>(offsets, data, ld, v, n, i, k0, acc)          U diagonals from k0, the one row i (may be >= n)
//   is_interior(g0, RW, omin, omax, n)                           the group of RW rows from g0 needs no test
//
// The host side of a family is DiaHost<Kernels>: the instantiated plans (R in
// {1, 2}, U in {1, 2, 4, 8}, load policy 2 or 8), the body of the plan rule and
// the launch.  `Kernels` names the family's __global__ template:
// Kernels::fn<R, U, NT>().
#pragma once
#include "cgx_matvec_core.h"

namespace cgx {

// R consecutive doubles from p: one 16-byte load when wide (R = 2), 8-byte loads otherwise.
template <int R, int NT>
__device__ __forceinline__ void load_piece(const double *__restrict__ p, bool wide, double (&d)[R]) {
    if constexpr (R == 2) {
        if (wide) {
            const d2 t = load_a<NT>(reinterpret_cast<const d2 *>(p));
            d[0] = t.x;
            d[1] = t.y;
        } else {
            d[0] = load_a<NT>(p);
            d[1] = load_a<NT>(p + 1);
        }
    } else {
        d[0] = load_a<NT>(p);
    }
}

// The body of a diagonal matVec kernel (its arguments are the kernel's).
template <class Terms, int R, int U, int NT>
__device__ __forceinline__ void dia_walk(const int32_t *__restrict__ offsets, const double *__restrict__ data,
                                         int64_t ld, int64_t n, int64_t ndiag, int vec,
                                         const double *__restrict__ v, double *__restrict__ out,
                                         const double *__restrict__ pown, double *dot_out, double *partials,
                                         unsigned *ticket, const int64_t *gate, int64_t *ts) {
    if (gate && *gate) return;  // the solve stopped in an earlier iteration (device-side gating)
    ts_start(ts);
    constexpr int RW = 64 * R;  // rows per wave
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int64_t ngroups = (n + RW - 1) / RW;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    int64_t omin = 0, omax = 0;  // min(0, min offset), max(0, max offset): wave-uniform
    for (int64_t k = 0; k < ndiag; ++k) {
        const int64_t o = offsets[k];
        omin = o < omin ? o : omin;
        omax = o > omax ? o : omax;
    }
    const int64_t kfull = ndiag - ndiag % U;
    double dacc[1] = {0.0};
    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t g0 = g * RW, i0 = g0 + (int64_t)lane * R;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        if (Terms::is_interior(g0, RW, omin, omax, n)) {
            for (int64_t k0 = 0; k0 < kfull; k0 += U)
                Terms::template interior<R, U, NT>(offsets, data, ld, v, i0, k0, vec != 0, acc);
            for (int64_t k0 = kfull; k0 < ndiag; ++k0)
                Terms::template interior<R, 1, NT>(offsets, data, ld, v, i0, k0, vec != 0, acc);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                for (int64_t k0 = 0; k0 < kfull; k0 += U)
                    Terms::template guarded<U, NT>(offsets, data, ld, v, n, i0 + r, k0, acc[r]);
                for (int64_t k0 = kfull; k0 < ndiag; ++k0)
                    Terms::template guarded<1, NT>(offsets, data, ld, v, n, i0 + r, k0, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (i0 + r < n) store_row(i0 + r, acc[r], out, pown, dacc[0]);
    }
    if (pown) grid_sum_last_block_n<1>(dacc, partials, ticket, dot_out, 1u);
    ts_end(ts);
}

// Both kernels' type, the same at every (R, U, policy).
using DiaFn = void (*)(const int32_t *, const double *, int64_t, int64_t, int64_t, int, const double *, double *,
                       const double *, double *, double *, unsigned *, const int64_t *, int64_t *);

template <class Kernels>
struct DiaHost {
    template <int R, int NT>
    static DiaFn pick_u(int U) {
        switch (U) {
            case 1: return Kernels::template fn<R, 1, NT>();
            case 2: return Kernels::template fn<R, 2, NT>();
            case 4: return Kernels::template fn<R, 4, NT>();
            case 8: return Kernels::template fn<R, 8, NT>();
            default: return nullptr;
        }
    }
    template <int NT>
    static DiaFn pick_nt(int R, int U) {
        return R == 1 ? pick_u<1, NT>(U) : R == 2 ? pick_u<2, NT>(U) : nullptr;
    }
    // The instantiated plan's kernel, or nullptr: R rows per lane (1 or 2), U diagonals in flight, load policy 2 or 8.
    static DiaFn pick(int R, int U, int nt) {
        return nt == 8 ? pick_nt<1>(R, U) : nt == 2 ? pick_nt<0>(R, U) : nullptr;
    }
    static bool plan_ok(int R, int U, int nt) { return pick(R, U, nt) != nullptr; }

    // The plan rule: the defaults (r0, u0, n0), then env = "R=..,U=..,nt=..,bpc=.." where it names an instantiated
    // plan, then the arguments (R / U <= 0, nt < 0, blocks_per_cu <= 0: not given), the defaults again where the
    // result is not instantiated; tag is pl.dia.
    static MatvecPlan plan(int device, int64_t n, int R, int U, int nt, int blocks_per_cu, int r0, int u0, int n0,
                           const char *env, int tag) {
        MatvecPlan pl;
        pl.csr = 1;
        pl.dia = tag;
        int r = r0, u = u0;
        pl.nt = n0;
        const int eR = env_opt(env, "R", r), eU = env_opt(env, "U", u), en = env_opt(env, "nt", pl.nt);
        if (plan_ok(eR, eU, en)) r = eR, u = eU, pl.nt = en;
        if (R > 0) r = R;
        if (U > 0) u = U;
        if (nt >= 0) pl.nt = nt;
        if (!plan_ok(r, u, pl.nt)) r = r0, u = u0, pl.nt = n0;
        pl.R = 64 * r;
        pl.U = u;
        pl.blocks = plan_grid(reinterpret_cast<const void *>(pick(r, u, pl.nt)), device, n, pl.R, 8, env, blocks_per_cu);
        return pl;
    }

    // The launch of a plan of this family (pl.dia == tag).
    static hipError_t launch(const MatvecPlan &pl, int tag, const int32_t *offsets, const double *data, int64_t ld,
                             int64_t n, int64_t ndiag, const double *v, double *out, const double *pown,
                             double *dot_out, const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
        if (n <= 0) return hipSuccess;
        if (pl.dia != tag || pl.R % 64 || !plan_ok(pl.R / 64, pl.U, pl.nt) || pl.blocks < 1 ||
            pl.blocks > kMaxRedBlocks || ndiag < 0 || ld < n)
            return hipErrorInvalidValue;
        const int vec = (ld % 2 == 0 && al16(data) && al16(v)) ? 1 : 0;  // the 16-byte loads of R = 2
        hipLaunchKernelGGL(pick(pl.R / 64, pl.U, pl.nt), dim3(pl.blocks), dim3(kNT), 0, s, offsets, data, ld, n, ndiag,
                           vec, v, out, pown, dot_out, ws.partials, ws.tickets + T_MATVEC, gate, ts);
        return hipGetLastError();
    }

    // Load the family's code object on the current device now (see preload_kernels).
    static hipError_t preload() {
        hipFuncAttributes a;
        return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(pick(1, 1, 2)));
    }
};

}  // namespace cgx
