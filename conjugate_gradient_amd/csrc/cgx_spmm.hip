// cgx_spmm.hip -- the sparse matVec of a cgx_create_csr_nrhs context: k_csr_mult_f64
// (cgx_csr_core.h, where the kernel, its order contract and the plan rule are)
// at the widths K = nrhs_width(nrhs) = 2, 4 and 8, a code object of its own.
#include "cgx_csr_core.h"

namespace cgx {

bool spmm_csr_plan_ok(int K, int T, int nt) { return csr_plan_ok<2, 4, 8>(K, T, nt); }

MatvecPlan plan_spmm_csr(int device, int64_t rows, int64_t nnz, int K, int T, int nt, int blocks_per_cu, bool f32) {
    return plan_csr<2, 4, 8>(device, rows, nnz, K, T, nt, blocks_per_cu, f32);
}

hipError_t spmm_csr_f64(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, int nrhs, const double *V, int64_t ldv, double *Out, int64_t ldo,
                        const double *pown, int64_t ldp, double *dot_out, const RedWs &ws, hipStream_t s,
                        const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    if (nrhs < 1 || nrhs > kMaxNrhs || pl.nrhs != nrhs_width(nrhs)) return hipErrorInvalidValue;
    return csr_mult_f64<2, 4, 8>(pl, pl.nrhs, row_ptr, col_idx, values, rows, nrhs, V, ldv, Out, ldo, pown, ldp,
                                 dot_out, ws, s, gate, ts);
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_spmm() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_csr_mult_f64<double, 8, 2, 1>));
}

}  // namespace cgx
