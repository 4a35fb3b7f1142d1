// cgx_pcg.hip -- diagonally preconditioned CG on cgx_create_csr contexts
// (cgx_set_precond / cgx_set_precond_diag, cgx_csr.hip): the start of the
// solve and the two update kernels with one more 8-byte stream each (minv),
// and the one-time extraction of 1 / diag(A) from the CSR arrays.
//
// z = minv o r is never stored: both update kernels form z_i = fl(minv_i r_i)
// from the minv and r they read anyway.  r.r and r.z come out of one pass
// (grid_sum_last_block_n<2>: each summed as the one-value reduction sums it).
//
// Contraction contract.  Every kernel below is a vec_pass (cgx_vector_core.h)
// whose body runs with fp contraction off (the pragma stands inside each
// body: it is lexical) and spells its fused operations out with the header's
// vfma / vmul / dot_acc, in the shapes hipcc gives the plain kernels' single
// spellings there (sub_r, axpy_x, next_p, elem_dot; read off the gfx950 ISA
// of cgx_vector.hip):
//   r_i   = fma(-alpha, Ap_i, r_i)               sub_r
//   x_i   = fma(alpha, p_i, x_i)                 axpy_x
//   z_i   = minv_i * r_i                         a rounded product
//   p_i   = fma(beta, p_i, z_i)                  next_p, z for r
//   pair  : acc = acc + fma(a.x, b.x, a.y * b.y) acc += elem_dot: r.r's, and r.z with b = z
//   tail  : acc = fma(a, b, acc)                 the odd last element
// so minv == 1 gives the plain kernels' bits, and minv == a power of two the
// same x (alpha absorbs 1 / c, p absorbs c).
#include "cgx_vector_core.h"

namespace cgx {
namespace {

// r = b - A x (Ax == nullptr: b - 0.0), p = minv o r, out[0] = r.r,
// out[stride] = r.z; block 0 resets the convergence record (k_residual_f64).
__global__ __launch_bounds__(kNT) void k_pcg_residual_f64(int64_t n, const double *__restrict__ b,
                                                          const double *__restrict__ Ax,
                                                          const double *__restrict__ minv, double *__restrict__ r,
                                                          double *__restrict__ p, double *out, int stride,
                                                          double *partials, unsigned *ticket, int64_t *clear2) {
#pragma clang fp contract(off)
    if (clear2 && blockIdx.x == 0 && threadIdx.x < 2) clear2[threadIdx.x] = 0;
    double acc[2] = {0.0, 0.0};
    const auto body = [&](int64_t i, auto io, auto bv, auto av, auto mv) {
#pragma clang fp contract(off)
        const auto ri = bv - av;
        const auto zi = vmul(mv, ri);
        io.st(r + i, ri);
        io.st(p + i, zi);
        acc[0] = dot_acc(acc[0], ri, ri);
        acc[1] = dot_acc(acc[1], ri, zi);
    };
    vec_pass<true, 0>(n, body, vin(b), vopt(Ax, Ax != nullptr), vin(minv));
    grid_sum_last_block_n<2>(acc, partials, ticket, out, 3u, stride);
}

// r -= alpha Ap (alpha = r.z_old / p.Ap); out[0] = r.r, out[stride] = r.z
// with z = minv o r  (k_update_r_f64 plus the minv stream: 32 B per row)
__global__ __launch_bounds__(kNT) void k_pcg_update_r_f64(int64_t n, double *__restrict__ r,
                                                          const double *__restrict__ Ap,
                                                          const double *__restrict__ minv, const double *rz_old,
                                                          const double *pAp, double *out, int stride,
                                                          double *partials, unsigned *ticket, const int64_t *gate) {
#pragma clang fp contract(off)
    if (gate && *gate) return;
    const double nalpha = -cg_ratio(*rz_old, *pAp);
    double acc[2] = {0.0, 0.0};
    const auto body = [&](int64_t i, auto io, auto rv, auto av, auto mv) {
#pragma clang fp contract(off)
        const auto ri = vfma(nalpha, av, rv);
        const auto zi = vmul(mv, ri);
        io.st(r + i, ri);
        acc[0] = dot_acc(acc[0], ri, ri);
        acc[1] = dot_acc(acc[1], ri, zi);
    };
    vec_pass<true, 2>(n, body, vin(r), vin(Ap), vin(minv));
    grid_sum_last_block_n<2>(acc, partials, ticket, out, 3u, stride);
}

// x += alpha p; then, if rr != nullptr and the loop goes on, p = z + beta p
// with z = minv o r recomputed and beta = r.z_new / r.z_old  (k_update_xp_f64
// plus the minv stream: 48 B per row).  The stopping decision is
// k_update_xp_f64's, on r.r: sqrt(*rr) < eps leaves p alone and records k + 1.
__global__ __launch_bounds__(kNT) void k_pcg_update_xp_f64(int64_t n, double *__restrict__ x, double *__restrict__ p,
                                                           const double *__restrict__ r,
                                                           const double *__restrict__ minv, const double *rz_old,
                                                           const double *pAp, const double *rr, const double *rz_new,
                                                           ConvArgs cv) {
#pragma clang fp contract(off)
    const StopStep st = gated_stop(cv, rr != nullptr, [&] { return rr ? *rr : 0.0; });
    if (!st.live) return;
    const bool upd_p = st.upd_p;
    const double rzo = *rz_old;
    const double alpha = cg_ratio(rzo, *pAp);
    const double beta = upd_p ? cg_ratio(*rz_new, rzo) : 0.0;
    const auto body = [&](int64_t i, auto io, auto xv, auto pv, auto rv, auto mv) {
#pragma clang fp contract(off)
        io.st(x + i, vfma(alpha, pv, xv));
        if (upd_p) io.st(p + i, vfma(beta, pv, vmul(mv, rv)));
    };
    vec_pass<true, 2>(n, body, vin(x), vin(p), vopt(r, upd_p), vopt(minv, upd_p));
}

// One-time set-up, one row per lane: d_i = the sum, from +0.0 in stored order,
// of row i's entries whose column is i; minv_i = 1.0 / d_i (fp64 division,
// correctly rounded).  A row with no such entry, or whose d_i is not finite or
// not > 0, stores d_i in place of the reciprocal (-0.0 when there is no entry:
// a sum started from +0.0 is never -0.0) and takes part in the atomicMin that
// leaves the lowest such row in *bad (the host set it to all ones).  The
// indices passed cgx_csr_check (cgx_set_csr), so every e is inside the arrays.
// VT = float (a float-valued context): each entry is widened exactly and d is
// the same double sum.
template <class VT>
__global__ __launch_bounds__(kNT) void k_csr_diag_minv(int64_t n, const int64_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ col_idx,
                                                       const VT *__restrict__ values, double *__restrict__ minv,
                                                       unsigned long long *bad) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kNT) {
        double d = 0.0;
        bool found = false;
        const int64_t e1 = row_ptr[i + 1];
        for (int64_t e = row_ptr[i]; e < e1; ++e)
            if ((int64_t)col_idx[e] == i) {
                d = d + (double)values[e];
                found = true;
            }
        const bool good = found && d > 0.0 && d < __builtin_inf();
        minv[i] = good ? 1.0 / d : found ? d : -0.0;
        if (!good) atomicMin(bad, (unsigned long long)i);
    }
}

}  // namespace

hipError_t pcg_residual_f64(int64_t n, const double *b, const double *Ax, const double *minv, double *r, double *p,
                            double *out, int stride, const RedWs &ws, hipStream_t s, int64_t *clear2) {
    if (!(al16(b) && al16(Ax) && al16(minv) && al16(r) && al16(p))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pcg_residual_f64, dim3(grid_vec(n)), dim3(kNT), 0, s, n, b, Ax, minv, r, p, out, stride,
                       ws.partials, ws.tickets + T_RESID, clear2);
    return hipGetLastError();
}

hipError_t pcg_update_r_f64(int64_t n, double *r, const double *Ap, const double *minv, const double *rz_old,
                            const double *pAp, double *out, int stride, const RedWs &ws, hipStream_t s,
                            const int64_t *gate) {
    if (!(al16(r) && al16(Ap) && al16(minv))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pcg_update_r_f64, dim3(grid_vec(n)), dim3(kNT), 0, s, n, r, Ap, minv, rz_old, pAp, out,
                       stride, ws.partials, ws.tickets + T_XR, gate);
    return hipGetLastError();
}

hipError_t pcg_update_xp_f64(int64_t n, double *x, double *p, const double *r, const double *minv,
                             const double *rz_old, const double *pAp, const double *rr, const double *rz_new,
                             hipStream_t s, double eps, int64_t k, int64_t *kdone, double *rrfinal, int64_t *hrec) {
    if (!(al16(x) && al16(p) && al16(r) && al16(minv))) return hipErrorInvalidValue;
    const ConvArgs cv = conv_args(eps, k, kdone, rrfinal, hrec);
    hipLaunchKernelGGL(k_pcg_update_xp_f64, dim3(grid_vec(n)), dim3(kNT), 0, s, n, x, p, r, minv, rz_old, pAp, rr,
                       rz_new, cv);
    return hipGetLastError();
}

hipError_t csr_diag_minv_f64(int64_t n, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                             double *minv, unsigned long long *bad, hipStream_t s) {
    if (values.f32)
        hipLaunchKernelGGL(k_csr_diag_minv<float>, dim3(grid_1d(n, kNT, 65536)), dim3(kNT), 0, s, n, row_ptr, col_idx,
                           static_cast<const float *>(values.p), minv, bad);
    else
        hipLaunchKernelGGL(k_csr_diag_minv<double>, dim3(grid_1d(n, kNT, 65536)), dim3(kNT), 0, s, n, row_ptr, col_idx,
                           static_cast<const double *>(values.p), minv, bad);
    return hipGetLastError();
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_pcg() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_csr_diag_minv<double>));
}

}  // namespace cgx
