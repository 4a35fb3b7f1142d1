// cgx_spmv.hip -- the sparse matVec of a cgx_create_csr context: k_csr_mult_f64
// (cgx_csr_core.h, where the kernel, its order contract and the plan rule are)
// at width K = 1, a code object of its own.
#include "cgx_csr_core.h"

namespace cgx {

bool spmv_csr_plan_ok(int T, int nt) { return csr_plan_ok<1>(1, T, nt); }

MatvecPlan plan_spmv_csr(int device, int64_t rows, int64_t nnz, int T, int nt, int blocks_per_cu, bool f32) {
    return plan_csr<1>(device, rows, nnz, 1, T, nt, blocks_per_cu, f32);
}

hipError_t spmv_csr_f64(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, const double *v, double *out, const double *pown, double *dot_out,
                        const RedWs &ws, hipStream_t s, const int64_t *gate, int64_t *ts) {
    if (rows <= 0) return hipSuccess;
    return csr_mult_f64<1>(pl, 1, row_ptr, col_idx, values, rows, /*nrhs=*/1, v, 0, out, 0, pown, 0, dot_out, ws, s,
                           gate, ts);
}

// Load this file's code object on the current device now (see preload_kernels).
hipError_t preload_spmv() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k_csr_mult_f64<double, 8, 1, 1>));
}

}  // namespace cgx
