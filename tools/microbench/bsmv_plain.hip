// bsmv_plain.hip -- the plain-layout variant of k_bsr_mult_f64 (csrc/cgx_bsmv.hip), for tools/bsmv_ab.py only.
//
// The library's kernel reads the values from tiles of 64 blocks, entry-major inside a tile, so that a wave's lanes
// read consecutive doubles.  This variant reads scipy's layout as it stands -- block q's entry e at q * BS^2 + e, each
// lane its own contiguous block, every load instruction strided by BS^2 * 8 bytes across the wave -- with the same
// lane mapping, trips in flight, load policies and summation order, so the A/B times the layout alone.  No fused dot,
// no gate.  BS = 3 and 4 (the block sizes the tool measures), T = 2 .. 64, load policy 2 (default) or 8
// (non-temporal).
//
// Built by the tool:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -o libbsmv_plain.so bsmv_plain.hip
// bsmv_timer_start / bsmv_timer_stop bracket launches on the null stream with two events, which is how the tool times
// this variant, the library's kernel-level cgx_spmv_bsr and cgx_spmv_csr alike.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kNT = 256;
typedef double d2 __attribute__((ext_vector_type(2)));

template <int BS>
constexpr int kU = BS == 2 ? 4 : BS <= 4 ? 2 : 1;  // cgx_bsmv.hip's kBsmvU

template <int NT, class V>
__device__ __forceinline__ V load_a(const V *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

template <int BS, int T, int NT>
__global__ __launch_bounds__(kNT) void k_bsr_mult_plain(const int64_t *__restrict__ brow_ptr,
                                                         const int32_t *__restrict__ bcol_idx,
                                                         const double *__restrict__ values, int64_t nb,
                                                         const double *__restrict__ v, double *__restrict__ out) {
    constexpr int RW = 64 / T, U = kU<BS>, E = BS * BS;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int sub = lane & (T - 1), rloc = lane / T;
    const int64_t ngroups = (nb + RW - 1) / RW;
    const int64_t wstride = (int64_t)gridDim.x * (kNT / 64);
    for (int64_t g = (int64_t)blockIdx.x * (kNT / 64) + wid; g < ngroups; g += wstride) {
        const int64_t I = g * RW + rloc;
        const bool live = I < nb;
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
                const double *ap = values + q * E;
#pragma unroll
                for (int m = 0; m < E; ++m) a[u][m] = ok ? load_a<NT>(ap + m) : 0.0;
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
            for (int i = 0; i < BS; ++i) out[I * BS + i] = acc[i];
        }
    }
}

using Fn = decltype(&k_bsr_mult_plain<3, 8, 0>);

template <int BS, int NT>
Fn pick_t(int T) {
    switch (T) {
        case 2: return k_bsr_mult_plain<BS, 2, NT>;
        case 4: return k_bsr_mult_plain<BS, 4, NT>;
        case 8: return k_bsr_mult_plain<BS, 8, NT>;
        case 16: return k_bsr_mult_plain<BS, 16, NT>;
        case 32: return k_bsr_mult_plain<BS, 32, NT>;
        case 64: return k_bsr_mult_plain<BS, 64, NT>;
        default: return nullptr;
    }
}
Fn pick(int bs, int T, int nt) {
    if (nt != 2 && nt != 8) return nullptr;
    if (bs == 3) return nt == 8 ? pick_t<3, 1>(T) : pick_t<3, 0>(T);
    if (bs == 4) return nt == 8 ? pick_t<4, 1>(T) : pick_t<4, 0>(T);
    return nullptr;
}

hipEvent_t g_ev[2] = {nullptr, nullptr};

}  // namespace

extern "C" {

// One launch on the null stream; the grid by plan_grid's rule (occupancy x CUs, at most what the block rows need).
// 0, -1 when (bs, T, nt) is not instantiated or v is misaligned for an even bs, -2 on a HIP error.
int bsmv_plain_launch(int bs, int T, int nt, int64_t nb, const void *brow_ptr, const void *bcol_idx, const void *values,
                      const void *v, void *out) {
    const Fn fn = pick(bs, T, nt);
    if (!fn || nb < 1 || (bs % 2 == 0 && (reinterpret_cast<uintptr_t>(v) & 15))) return -1;
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return -2;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(fn), kNT, 0) != hipSuccess ||
        per_cu <= 0)
        per_cu = 8;
    const int RW = 64 / T;
    const int64_t groups = (nb + RW - 1) / RW, need = (groups + 3) / 4;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(need, std::min<int64_t>((int64_t)per_cu * cus, 8192)));
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(kNT), 0, nullptr, static_cast<const int64_t *>(brow_ptr),
                       static_cast<const int32_t *>(bcol_idx), static_cast<const double *>(values), nb,
                       static_cast<const double *>(v), static_cast<double *>(out));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int bsmv_timer_start() {
    for (auto &e : g_ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return -2;
    return hipEventRecord(g_ev[0], nullptr) == hipSuccess ? 0 : -2;
}

// milliseconds since bsmv_timer_start on the null stream (waits for the work between them); < 0 on a HIP error
float bsmv_timer_stop() {
    float ms = -1.0f;
    if (hipEventRecord(g_ev[1], nullptr) != hipSuccess || hipEventSynchronize(g_ev[1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g_ev[0], g_ev[1]) != hipSuccess)
        return -1.0f;
    return ms;
}

}  // extern "C"
