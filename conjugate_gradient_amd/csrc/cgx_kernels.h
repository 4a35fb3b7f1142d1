// cgx_kernels.h -- host-side launchers for the CDNA4 (gfx950) CG kernels.
// Internal to libcgx.so; the public boundary is include/cgx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cgx {

// Scratch needed by the last-block reductions (one set per stream in use).
struct RedWs {
    double *partials;      // >= kMaxRedBlocks doubles
    unsigned *tickets;     // kTickets counters, zero at rest
};
constexpr int kMaxRedBlocks = 8192;
// Most partials a scalar combine takes (>= kMaxShards, the rank limit).
constexpr int kMaxCombine = 64;
constexpr int kTickets = 8;
enum Ticket { T_MATVEC = 0, T_RESID = 1, T_XR = 2, T_DOT = 3, T_REF_MV = 4 };

// ---- the multi-shard exchange in one process (several row blocks, LOCAL) ---
// Pointers to every shard's copy of something (its p slice, its scalar slot),
// in shard order; passed by value.  On distinct devices they are peer
// pointers (access enabled at context creation): the kernels below run on the
// CONSUMING shard's stream and only read peers' memory -- the same pull a
// hipMemcpyPeerAsync on that stream does -- after the stream has waited for
// the producers' events.
constexpr int kMaxPeers = 32;
struct PeerTable {
    const char *p[kMaxPeers];
};
// dst[q * slice_bytes ...] = src.p[q][0 .. slice_bytes) for every q < cnt
// except q == skip (the consumer's own slice, already in place; skip < 0
// copies every slice): the allgather of p (or of x) in one launch instead of
// cnt - 1 peer copies.
hipError_t gather_slices(const PeerTable &src, int cnt, int skip, int64_t slice_bytes, char *dst, hipStream_t s);
// The indexed form of gather_slices for a sparse A's row blocks (cgx_create_csr_multi): of source q's slice of
// nloc doubles only the entries its list names, dst[q * nloc + j] = src.p[q][j] for the j in
// idx[lists.off[q] .. lists.off[q + 1]) (offsets into the slice, each once).  A source whose list has nloc
// entries, and source `whole` (the consumer's own x; < 0: none), is the contiguous slice, no index reads;
// source `skip` (< 0: none) and an empty list move nothing.  The offsets are not range-checked: the host
// builds them from a checked structure (cgx_csr.hip).
struct GatherLists {
    int64_t off[kMaxPeers + 1];
};
hipError_t gather_indexed(const PeerTable &src, int cnt, int skip, int whole, const GatherLists &lists,
                          const int32_t *idx, int64_t nloc, double *dst, hipStream_t s);
// *out = the cnt partials src.p[q] (fp64), summed in q order: the rank-order
// combine of exchange_scalar read straight from each shard's slot.
hipError_t combine_peers_f64(const PeerTable &src, int cnt, double *out, hipStream_t s);
// F32_REF: the float partials in rank order or (mpich) MPICH's MPI_Allreduce order.
hipError_t combine_peers_f32(const PeerTable &src, int cnt, float *out, hipStream_t s, bool mpich);
// The fp64 combine folded into the kernel that consumes the scalar (no
// launch of its own): every block sums the cnt partials src.p[q] in q order
// (k_combine_peers' sum, so the same bits) and uses it in place of the
// global slot; block 0 also stores it to *out (the global slot) for later
// kernels and the host.  cnt = 0: none (the kernel reads the slot).
struct PeerSum {
    PeerTable src;
    int cnt;
    double *out;
};
// The F32_REF counterpart: the cnt float partials combined in MPICH's
// MPI_Allreduce order (k_combine_peers<float>'s mpich form, the same adds),
// folded into k_dot_ref_f32_blk<kDotXR> (p.Ap) and k_update_p_ref_f32 (r.r).
struct PeerSumF32 {
    PeerTable src;
    int cnt;
    float *out;
};

// CGX_PHASES in-kernel timestamps: a kernel given `ts` stores block 0's entry
// time in ts[0] and block b's exit time in ts[1 + b] (b < kTsMaxBlocks), on
// the device's constant wall clock (hipDeviceAttributeWallClockRate).  No
// event packets between the kernels, so the timeline being measured is the
// one that runs without CGX_PHASES.
constexpr int kTsMaxBlocks = 2047;
constexpr int kTsSlot = kTsMaxBlocks + 1;  // int64 per kernel slot

// Geometry of the fp64 row-streaming matVec, chosen once per (device, rows).
struct MatvecPlan {
    int R = 4;        // rows per wave
    int U = 4;        // 128-column chunks in flight per row
    int nt = 1;       // non-temporal loads of A
    int blocks = 0;   // grid (256-thread blocks), grid-stride over row groups
    int small = 0;    // > 0: k_matvec_small_f64 with this many threads per block (vector in LDS)
    int a32 = 0;      // 1: k_matvec_a32's plan (float A; U counts 256-column chunks, nt is 2 or 8)
    int nrhs = 0;     // > 0: k_matvec_nrhs_f64's plan for this many vectors per pass (2, 4 or 8; nt is 2 or 8)
    int csr = 0;      // 1: k_csr_mult_f64's plan (R = 64 / T rows per wave, U = 1, nt is 2 or 8)
    int bsr = 0;      // > 0 (with csr = 1): k_bsr_mult_f64's plan for this block size (R = 64 / T block rows per wave)
    int dia = 0;      // 1 (with csr = 1): k_dia_mult_f64's plan (R = 64 or 128 rows per wave, U diagonals in flight);
                      // 2: k_dia_sym_mult_f64's, the same ranges (U counts stored diagonals)
};
// R/U/nt/blocks_per_cu <= 0 pick the defaults (env CGX_MV_PLAN="R=..,U=..,nt=..,bpc=.."
// may override).
// cols > 0 (the row length): fewer than 8 whole 128-column chunks per row
// take U = 4 or 2, so all of a row's loads are issued at once.
MatvecPlan plan_matvec_f64(int device, int64_t rows, int R = 0, int U = 0, int nt = -1,
                           int blocks_per_cu = 0, int64_t cols = 0);
// The LDS-staged matVec of small systems (cgx_matvec.hip k_matvec_small_f64):
// rows of lda columns, 2048 <= lda <= 8192; small = 0 (not applicable)
// otherwise.  CGX_MV_SMALL=0 turns it off; CGX_SMALL_PLAN="threads=..,U=..,nt=.."
// picks the block size (512, 1024), chunks per step (4, 8) and A's load policy.
MatvecPlan plan_matvec_small_f64(int device, int64_t rows, int64_t lda);
// What the plans of the row-streaming family share (cgx_matvec.hip).
// The grid of kernel fn with R rows per wave: its occupancy (per_cu_fallback
// blocks per CU when the query fails), then env's "bpc", then blocks_per_cu
// (> 0), times the CUs; at most the blocks the row groups need and kMaxRedBlocks.
int plan_grid(const void *fn, int device, int64_t rows, int R, int per_cu_fallback, const char *env, int blocks_per_cu);
// (R, U, nt) of a family whose plans are a list (ok(pl.nrhs, R, U, nt) says
// whether one is instantiated): env's plan when it names one, then the
// arguments (R, U > 0, nt >= 0), then (fallback_R, fallback_U, 8).
void plan_listed(MatvecPlan &pl, const char *env, int R, int U, int nt, bool (*ok)(int K, int R, int U, int nt),
                 int fallback_R, int fallback_U);
// The columns that go through the vector path: the whole chunks of `chunk`
// columns when no pointer has a bit of its alignment mask set (misaligned: the
// OR of those bits) and the pitch keeps every row aligned; otherwise 0, every
// column through the scalar tail.
inline int64_t matvec_vec_cols(uintptr_t misaligned, bool pitch_ok, int64_t cols, int chunk) {
    return (misaligned == 0 && pitch_ok) ? (cols & ~int64_t(chunk - 1)) : 0;
}

// ---- fp64 -------------------------------------------------------------------
// out[i] = sum_j A[i*lda+j] v[j]; if pown != nullptr also *dot_out = pown . out
// (last-block reduction, fixed order).
// gate (optional): device word; when non-zero the kernel returns at once
// (device-side convergence gating of queued iterations).
hipError_t matvec_f64(const MatvecPlan &pl, const double *A, int64_t lda, int64_t rows,
                      int64_t cols, const double *v, double *out, const double *pown,
                      double *dot_out, const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr,
                      int64_t *ts = nullptr);
// Columns [col_first, col_first+col_count) mod cols (all multiples of 128,
// cols = the padded width): out[i] = (accumulate ? out[i] : 0) + partial row
// sum; optional fused dot as above.  Used to overlap the p exchange with the
// shard's own column block.  col_seg > 0 (not with accumulate): the first
// col_seg columns of the range and the rest are summed separately and added
// (own + rest) -- the bits of a col_seg launch followed by an accumulating
// launch of the rest, in one launch (the unoverlapped iteration of an
// aligned row block, so both forms give the same x).
hipError_t matvec_f64_cols(const MatvecPlan &pl, const double *A, int64_t lda, int64_t rows, int64_t cols,
                           int64_t col_first, int64_t col_count, bool accumulate, const double *v, double *out,
                           const double *pown, double *dot_out, const RedWs &ws, hipStream_t s,
                           const int64_t *gate = nullptr, int64_t *ts = nullptr, int64_t col_seg = 0);
// CGX_A_F32 (cgx_matvec_a32.hip): A stored as float, widened exactly, fp64
// FMAs; v, out, pown and the fused dot are double as above.  The plan comes
// from plan_matvec_a32: R/U/nt <= 0 / < 0 pick the defaults (env
// CGX_MV_A32_PLAN="R=..,U=..,nt=..,bpc=.." may override with an instantiated
// plan); matvec_a32_plan_ok says whether (R, U, nt) is instantiated.
bool matvec_a32_plan_ok(int R, int U, int nt);
MatvecPlan plan_matvec_a32(int device, int64_t rows, int R = 0, int U = 0, int nt = -1, int blocks_per_cu = 0,
                           int64_t cols = 0);
hipError_t matvec_a32(const MatvecPlan &pl, const float *A, int64_t lda, int64_t rows, int64_t cols, const double *v,
                      double *out, const double *pown, double *dot_out, const RedWs &ws, hipStream_t s,
                      const int64_t *gate = nullptr, int64_t *ts = nullptr);
// ---- several right-hand sides per pass over A (cgx_matvec_nrhs.hip) -----------
// Out[j*ldo + i] = sum_c A[i*lda + c] V[j*ldv + c] for j < nrhs: every element
// of A loaded once and multiplied by K = nrhs_width(nrhs) vector elements (2,
// 4 or 8; columns nrhs..K-1 re-read column 0 and are not stored).  Each
// column's row sum adds in k_matvec_f64's order, so it is matvec_f64's result
// on that column bit for bit under every plan.  pown != nullptr: also
// dot_out[j] = pown[j*ldp ..] . Out[j*ldo ..] for every j < nrhs (fixed order).
constexpr int kMaxNrhs = 8;
inline int nrhs_width(int nrhs) { return nrhs <= 2 ? 2 : nrhs <= 4 ? 4 : 8; }
// Reduction scratch of the nrhs kernels: kMaxNrhs * kMaxRedBlocks partials, kNrhsTickets counters.
constexpr int kNrhsTickets = 4;
enum NrhsTicket { TN_MATVEC = 0, TN_RESID = 1, TN_R = 2, TN_DOT = 3 };
// The instantiated (K, R, U, policy): the policy is 2 (default-policy loads) or
// 8 (non-temporal), both software-pipelined.
bool matvec_nrhs_plan_ok(int K, int R, int U, int nt);
// The plan for K vectors per pass: R/U/nt <= 0 / < 0 pick the defaults (env
// CGX_MV_NRHS_PLAN="R=..,U=..,nt=..,bpc=.." may override with an instantiated plan).
MatvecPlan plan_matvec_nrhs(int device, int64_t rows, int K, int R = 0, int U = 0, int nt = -1, int blocks_per_cu = 0,
                            int64_t cols = 0);
hipError_t matvec_nrhs_f64(const MatvecPlan &pl, const double *A, int64_t lda, int64_t rows, int64_t cols, int nrhs,
                           const double *V, int64_t ldv, double *Out, int64_t ldo, const double *pown, int64_t ldp,
                           double *dot_out, const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr,
                           int64_t *ts = nullptr);
// The scalars of an nrhs solve, on the device: r.r and p.Ap rings of 4 as the
// one-system slots (cgx_ctx.h), per column; the true-residual dots; and the
// per-column stopping record -- kdone[j] = k+1 and rrfinal[j] = r_j.r_j at the
// iteration k that stopped column j (0: still iterating), alldone = k+1 of the
// iteration that stopped the last column (the gate of every later launch).
struct NrhsScal {
    double rr[4][kMaxNrhs], pap[4][kMaxNrhs];
    double tr[kMaxNrhs], tb[kMaxNrhs];
    int64_t kdone[kMaxNrhs];
    double rrfinal[kMaxNrhs];
    int64_t alldone, pad_;
};
// The K-column vector kernels.  Column j of every vector starts at j*ld
// doubles (ld even, bases 16-B aligned).  A column whose kdone is set is
// frozen: no kernel writes its x, r, p or scalars again.
// r_j = b_j - Ax_j (Ax == nullptr: b_j - 0.0); p_j = r_j when p != nullptr;
// out[j] = r_j.r_j.  clear != nullptr: the stopping record of *clear and the
// host-mapped word *hrec are reset (the start of a solve).
hipError_t nrhs_residual_f64(int64_t n, int64_t ld, int nrhs, const double *b, const double *Ax, double *r, double *p,
                             double *out, NrhsScal *clear, int64_t *hrec, const RedWs &ws, hipStream_t s);
// out[j] = a_j . b_j
hipError_t nrhs_dot_f64(int64_t n, int64_t ld, int nrhs, const double *a, const double *b, double *out,
                        const RedWs &ws, hipStream_t s);
// iteration k: r_j -= alpha_j Ap_j, sc->rr[ring(k+1)][j] = r_j.r_j, alpha_j = rr[ring(k)][j] / pap[ring(k)][j]
hipError_t nrhs_update_r_f64(int64_t n, int64_t ld, int nrhs, int64_t k, double *r, const double *Ap, NrhsScal *sc,
                             const RedWs &ws, hipStream_t s);
// iteration k: x_j += alpha_j p_j; then the stopping decision per column
// (eps >= 0: sqrt(r_j.r_j) < eps records kdone[j] = k+1, rrfinal[j], and, when
// every column has stopped, alldone and the host-mapped hrec[0] = k+1); a
// column that goes on gets p_j = r_j + beta_j p_j.
hipError_t nrhs_update_xp_f64(int64_t n, int64_t ld, int nrhs, int64_t k, double eps, double *x, double *p,
                              const double *r, NrhsScal *sc, int64_t *hrec, hipStream_t s);

// ---- sparse A in CSR storage (cgx_spmv.hip) --------------------------------------
// out[i] = sum over e in [row_ptr[i], row_ptr[i+1]) of values[e] * v[col_idx[e]],
// entries in stored order, T = 64 / pl.R lanes per row (the order contract is
// in cgx_csr_core.h); pown != nullptr: also *dot_out = pown . out (fixed order
// for a fixed grid).  The indices are not range-checked here (cgx_csr_check).
// The instantiated (T, policy): T in {2, 4, 8, 16, 32, 64}, policy 2 or 8.
bool spmv_csr_plan_ok(int T, int nt);
// The values of a CSR matrix: double[nnz], or float[nnz] (cgx_set_csr_f32),
// which every kernel below widens exactly with (double) before the same fp64
// operations in the same order: a float-valued launch gives the bits of a
// double-valued one on (double)values[e].  A pointer converts by its type.
struct CsrValues {
    const void *p;
    bool f32;
    CsrValues(const double *d) : p(d), f32(false) {}
    CsrValues(const float *f) : p(f), f32(true) {}
    CsrValues(const void *q, bool is_f32) : p(q), f32(is_f32) {}
};
// T <= 0 / nt < 0 / blocks_per_cu <= 0 pick the defaults (T from the mean row
// length nnz / rows, 8 when nnz < 0; env CGX_SPMV_PLAN="T=..,nt=..,bpc=.." may override with an
// instantiated plan).  f32: the grid comes from the float-valued kernel's
// occupancy; the default T is the same for both value types.
MatvecPlan plan_spmv_csr(int device, int64_t rows, int64_t nnz, int T = 0, int nt = -1, int blocks_per_cu = 0,
                         bool f32 = false);
hipError_t spmv_csr_f64(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, const double *v, double *out, const double *pown, double *dot_out,
                        const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr, int64_t *ts = nullptr);

// ---- sparse A in block (BSR) storage (cgx_bsmv.hip) --------------------------------
// out[I bs + i] = sum over the blocks q in [brow_ptr[I], brow_ptr[I+1]) and j < bs of
// B_q[i][j] * v[bcol_idx[q] bs + j], blocks in stored order, j ascending, T = 64 / pl.R
// lanes per block row (the order contract and the device layout of the values are in
// cgx_bsmv.hip); pown != nullptr: also *dot_out = pown . out (fixed order for a fixed
// grid).  `tiled` holds bsr_tiled_count(nnzb, bs) doubles in the tiled layout
// (bsr_tile_values_f64 re-lays the host layout: block after block, row-major inside
// one).  The indices are not range-checked here (cgx_bsr_check); v is 16-byte aligned
// when bs is even (hipErrorInvalidValue otherwise).
// The instantiated (bs, T, policy): bs in 2..8, T in {2, 4, 8, 16, 32, 64}, policy 2 or 8.
constexpr int kMaxBsrBlock = 8;
inline int64_t bsr_tiled_count(int64_t nnzb, int bs) { return (nnzb + 63) / 64 * 64 * bs * bs; }
bool spmv_bsr_plan_ok(int bs, int T, int nt);
// T <= 0 / nt < 0 / blocks_per_cu <= 0 pick the defaults (T from the mean blocks per
// block row nnzb / nb, 8 when nnzb < 0; env CGX_BSMV_PLAN="T=..,nt=..,bpc=.." may
// override with an instantiated plan).  pl.csr = 1, pl.bsr = bs.
MatvecPlan plan_spmv_bsr(int device, int64_t nb, int64_t nnzb, int bs, int T = 0, int nt = -1, int blocks_per_cu = 0);
hipError_t spmv_bsr_f64(const MatvecPlan &pl, int bs, const int64_t *brow_ptr, const int32_t *bcol_idx,
                        const double *tiled, int64_t nb, const double *v, double *out, const double *pown,
                        double *dot_out, const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr,
                        int64_t *ts = nullptr);
hipError_t bsr_tile_values_f64(int64_t nnzb, int bs, const double *values, double *tiled, hipStream_t s);
// The preconditioners' one-time extraction from the BSR arrays (values in the host
// layout), bit for bit what csr_diag_minv_f64 / csr_diag_blocks_f64 (below) give on
// the expanded matrix -- row I bs + i's entries block after block in stored order, j
// ascending inside a block; pbs: the preconditioner's block size, any of 2..kMaxPcBlock.
hipError_t bsr_diag_minv_f64(int64_t n, int bs, const int64_t *brow_ptr, const int32_t *bcol_idx, const double *values,
                             double *minv, unsigned long long *bad, hipStream_t s);
hipError_t bsr_diag_blocks_f64(int64_t n, int bs, int pbs, const int64_t *brow_ptr, const int32_t *bcol_idx,
                               const double *values, double *D, hipStream_t s);

// ---- sparse A held by diagonals (cgx_dia.hip) --------------------------------------
// out[i] = sum over k < ndiag with 0 <= i + offsets[k] < n, in stored order, of
// data[k * ld + i + offsets[k]] * v[i + offsets[k]], one accumulator per row from
// +0.0 (the order contract is in cgx_dia.hip); pown != nullptr: also *dot_out =
// pown . out (fixed order for a fixed rows per wave and grid).  ld >= n; slots of
// data that hold no entry of A are never read.  The offsets are not range-checked
// here (cgx_dia_check), but an offset outside (-n, n) adds no term and reads nothing
// outside the arrays.  The 16-byte loads of R = 2 are used when ld is even and data
// and v are 16-byte aligned, 8-byte loads otherwise: the same bits.
// The instantiated (R, U, policy): rows per lane R in {1, 2} (pl.R = 64 R), U in
// {1, 2, 4, 8}, policy 2 or 8.
bool spmv_dia_plan_ok(int R, int U, int nt);
// R / U <= 0, nt < 0, blocks_per_cu <= 0 pick the defaults (env
// CGX_DIA_PLAN="R=..,U=..,nt=..,bpc=.." may override with an instantiated plan; its R
// counts rows per lane).  pl.csr = 1, pl.dia = 1.
MatvecPlan plan_spmv_dia(int device, int64_t n, int64_t ndiag, int R = 0, int U = 0, int nt = -1,
                         int blocks_per_cu = 0);
hipError_t spmv_dia_f64(const MatvecPlan &pl, const int32_t *offsets, const double *data, int64_t ld, int64_t n,
                        int64_t ndiag, const double *v, double *out, const double *pown, double *dot_out,
                        const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr, int64_t *ts = nullptr);
// The preconditioners' one-time extraction from the diagonals, bit for bit what
// csr_diag_minv_f64 / csr_diag_blocks_f64 (below) give on the expanded matrix -- row
// i's entries diagonal after diagonal in stored order, in-range terms only.
hipError_t dia_diag_minv_f64(int64_t n, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld,
                             double *minv, unsigned long long *bad, hipStream_t s);
hipError_t dia_diag_blocks_f64(int64_t n, int pbs, int64_t ndiag, const int32_t *offsets, const double *data,
                               int64_t ld, double *D, hipStream_t s);

// ---- symmetric A held by its upper diagonals (cgx_dia_sym.hip) ----------------------
// offsets >= 0, data[k * ld + j] = A[j - o][j] for j in [o, n), the stored diagonal of
// offset o > 0 also standing for the diagonal -o.  out[i] = from +0.0, for k in stored
// order, fma(data[k][i + o], v[i + o], .) where o > 0 and i + o < n, then
// fma(data[k][i], v[i - o], .) where i - o >= 0: bit for bit spmv_dia_f64 on the
// expansion (o, then -o), the fused pown . out included at the same rows per wave and
// grid.  Slots outside [o, n) are never read; an offset outside [0, n) adds no term
// and reads nothing outside the arrays.  The 16-byte loads of R = 2 as spmv_dia_f64's.
// The instantiated (R, U, policy) are spmv_dia_f64's: R in {1, 2}, U in {1, 2, 4, 8}
// stored diagonals in flight, policy 2 or 8 (of the values' last use: the lower piece
// and the offset-0 diagonals; the first use is a default-policy load).
bool spmv_dia_sym_plan_ok(int R, int U, int nt);
// As plan_spmv_dia, under CGX_DIA_SYM_PLAN="R=..,U=..,nt=..,bpc=..".  pl.csr = 1, pl.dia = 2.
MatvecPlan plan_spmv_dia_sym(int device, int64_t n, int64_t ndiag, int R = 0, int U = 0, int nt = -1,
                             int blocks_per_cu = 0);
hipError_t spmv_dia_sym_f64(const MatvecPlan &pl, const int32_t *offsets, const double *data, int64_t ld, int64_t n,
                            int64_t ndiag, const double *v, double *out, const double *pown, double *dot_out,
                            const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr, int64_t *ts = nullptr);
// The block preconditioner's one-time extraction, bit for bit what csr_diag_blocks_f64
// gives on the expansion (1 / diag(A) is dia_diag_minv_f64's: only offset 0 counts).
hipError_t dia_sym_diag_blocks_f64(int64_t n, int pbs, int64_t ndiag, const int32_t *offsets, const double *data,
                                   int64_t ld, double *D, hipStream_t s);

// ---- several right-hand sides on a CSR matrix (cgx_spmm.hip) ----------------------
// Out[j*ldo + i] = sum over row i's entries of values[e] * V[j*ldv + col_idx[e]]
// for j < nrhs: values and col_idx loaded once per entry and multiplied by
// K = nrhs_width(nrhs) gathered elements.  Each column sums in spmv_csr_f64's
// order at the same T = 64 / pl.R (both are k_csr_mult_f64, cgx_csr_core.h), so
// it is spmv_csr_f64's result on that column bit for bit.  pown != nullptr:
// also dot_out[j] = pown[j*ldp ..] . Out[j*ldo ..] for every j < nrhs (ws as
// the nrhs kernels': kMaxNrhs * kMaxRedBlocks partials).  The indices are not
// range-checked here.
// The instantiated (K, T, policy): K in {2, 4, 8}, T in {2, .., 64}, policy 2 or 8.
bool spmm_csr_plan_ok(int K, int T, int nt);
// T <= 0 / nt < 0 / blocks_per_cu <= 0 pick the defaults (T from the mean row
// length nnz / rows, 8 when nnz < 0; env CGX_SPMM_PLAN="T=..,nt=..,bpc=.."
// may override with an instantiated plan).  pl.nrhs = K, pl.csr = 1.  f32 as
// plan_spmv_csr's.
MatvecPlan plan_spmm_csr(int device, int64_t rows, int64_t nnz, int K, int T = 0, int nt = -1, int blocks_per_cu = 0,
                         bool f32 = false);
hipError_t spmm_csr_f64(const MatvecPlan &pl, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                        int64_t rows, int nrhs, const double *V, int64_t ldv, double *Out, int64_t ldo,
                        const double *pown, int64_t ldp, double *dot_out, const RedWs &ws, hipStream_t s,
                        const int64_t *gate = nullptr, int64_t *ts = nullptr);

// ---- diagonally preconditioned CG on CSR contexts (cgx_pcg.hip) ---------------------
// minv = the preconditioner's n positive values; z = minv o r is formed in
// registers, never stored.  Both sums of a kernel come out of one pass: r.r to
// out[0], r.z to out[stride] (ws.partials holds 2 * kMaxRedBlocks doubles).
// Every pointer is 16-byte aligned (hipErrorInvalidValue otherwise).
// r = b - Ax (Ax == nullptr: b - 0.0); p = minv o r; clear2 as residual_f64's.
hipError_t pcg_residual_f64(int64_t n, const double *b, const double *Ax, const double *minv, double *r, double *p,
                            double *out, int stride, const RedWs &ws, hipStream_t s, int64_t *clear2 = nullptr);
// r -= alpha Ap with alpha = *rz_old / *pAp
hipError_t pcg_update_r_f64(int64_t n, double *r, const double *Ap, const double *minv, const double *rz_old,
                            const double *pAp, double *out, int stride, const RedWs &ws, hipStream_t s,
                            const int64_t *gate = nullptr);
// x += alpha p; then (rr != nullptr) p = minv o r + (*rz_new / *rz_old) p.  The
// stopping decision is update_xp_f64's, on *rr.
hipError_t pcg_update_xp_f64(int64_t n, double *x, double *p, const double *r, const double *minv,
                             const double *rz_old, const double *pAp, const double *rr, const double *rz_new,
                             hipStream_t s, double eps = -1.0, int64_t k = 0, int64_t *kdone = nullptr,
                             double *rrfinal = nullptr, int64_t *hrec = nullptr);
// minv[i] = 1.0 / d_i, d_i = the sum in stored order of row i's entries in
// column i.  A row without one, or with d_i not finite or not > 0, stores d_i
// instead (-0.0: no entry) and lowers *bad (preset to all ones) to its index.
hipError_t csr_diag_minv_f64(int64_t n, const int64_t *row_ptr, const int32_t *col_idx, CsrValues values,
                             double *minv, unsigned long long *bad, hipStream_t s);

// ---- block-Jacobi preconditioned CG on CSR contexts (cgx_pcg_block.hip) --------------
// W = the nblk = ceil(n / bs) inverse diagonal blocks, 2 <= bs <= kMaxPcBlock;
// entry (i, j) of block k at W[(i * bs + j) * wld + k], wld >= nblk.  z = W r is
// formed block by block (the order is in cgx.h, "Sparse A") and stored by the r
// update for the x/p update.  Sums, slots and clear2 as the diagonal kernels'.
// The vectors are 16-byte aligned (hipErrorInvalidValue otherwise, or a bs
// outside the range).
constexpr int kMaxPcBlock = 8;
// r = b - Ax (Ax == nullptr: b - 0.0); p = W r
hipError_t pcgb_residual_f64(int bs, int64_t n, const double *b, const double *Ax, const double *W, int64_t wld,
                             double *r, double *p, double *out, int stride, const RedWs &ws, hipStream_t s,
                             int64_t *clear2 = nullptr);
// r -= alpha Ap with alpha = *rz_old / *pAp; z = W r
hipError_t pcgb_update_r_f64(int bs, int64_t n, double *r, const double *Ap, const double *W, int64_t wld, double *z,
                             const double *rz_old, const double *pAp, double *out, int stride, const RedWs &ws,
                             hipStream_t s, const int64_t *gate = nullptr);
// x += alpha p; then (rr != nullptr) p = z + (*rz_new / *rz_old) p.  The
// stopping decision is update_xp_f64's, on *rr.
hipError_t pcgb_update_xp_f64(int64_t n, double *x, double *p, const double *z, const double *rz_old,
                              const double *pAp, const double *rr, const double *rz_new, hipStream_t s,
                              double eps = -1.0, int64_t k = 0, int64_t *kdone = nullptr, double *rrfinal = nullptr,
                              int64_t *hrec = nullptr);
// D[(k * bs + i) * bs + j] = the sum in stored order of row k bs + i's entries in
// column k bs + j, +0.0 where there is none (nblk * bs * bs doubles).
hipError_t csr_diag_blocks_f64(int64_t n, int bs, const int64_t *row_ptr, const int32_t *col_idx,
                               CsrValues values, double *D, hipStream_t s);

// r = b - Ax; p = r (if p); *rr_out = r.r (if rr_out).  Ax == nullptr: Ax = 0
// (r = b - 0.0).  clear2: two int64 the kernel zeroes (the convergence record).
hipError_t residual_f64(int64_t n, const double *b, const double *Ax, double *r, double *p,
                        double *rr_out, const RedWs &ws, hipStream_t s, int64_t *clear2 = nullptr);
// alpha = *rsold / *pAp; x += alpha p; r -= alpha Ap; *rr_out = r.r
hipError_t update_xr_f64(int64_t n, double *x, double *r, const double *p, const double *Ap,
                         const double *rsold, const double *pAp, double *rr_out,
                         const RedWs &ws, hipStream_t s);
// p = r + (*rr / *rsold) p
hipError_t update_p_f64(int64_t n, double *p, const double *r, const double *rr,
                        const double *rsold, hipStream_t s);
// Solver split of the updates: r -= alpha Ap with *rr_out = r.r; then
// x += alpha p and (rr != nullptr) p = r + (*rr / *rsold) p; alpha = *rsold / *pAp.
// With kdone != nullptr update_xp also decides sqrt(*rr) < eps on the device:
// on convergence it skips the p update and stores *kdone = k+1, *rrfinal = *rr
// (and the same pair into hrec[0..1], host-mapped memory, when hrec != nullptr);
// once *kdone is in (0, k] both kernels (update_r via gate) do nothing.
hipError_t update_r_f64(int64_t n, double *r, const double *Ap, const double *rsold, const double *pAp,
                        double *rr_out, const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr,
                        int64_t *ts = nullptr, const PeerSum *pap_sum = nullptr);
// The two-launch iteration's update (one GPU, small n): x += alpha p;
// r -= alpha Ap; *rr_out = r.r; then (last block) the stopping decision as
// update_xp's, and unless stopped p = r + (*rr_out / *rsold) p.
hipError_t update_xrp_f64(int64_t n, double *x, double *r, double *p, const double *Ap, const double *rsold,
                          const double *pAp, double *rr_out, const RedWs &ws, hipStream_t s, const int64_t *gate,
                          double eps, int64_t k, int64_t *kdone, double *rrfinal, int64_t *hrec,
                          int64_t *ts = nullptr);
// The folded two-launch iteration (one GPU, small n): the matVec forms
// p_k = r + (*rr_new / *rr_old) p_{k-1} for the chunks it multiplies, stores
// p_k's own rows into pnew and fuses *dot_out = p_k . out; then update_xr_stop
// does x += alpha p_k, r -= alpha Ap, *rr_out = r.r and the stopping decision.
hipError_t matvec_fold_f64(const MatvecPlan &pl, const double *A, int64_t lda, int64_t rows, int64_t cols,
                           const double *r, const double *pold, double *pnew, const double *rr_new,
                           const double *rr_old, double *out, double *dot_out, const RedWs &ws, hipStream_t s,
                           const int64_t *gate = nullptr, int64_t *ts = nullptr);
hipError_t update_xr_stop_f64(int64_t n, double *x, double *r, const double *p, const double *Ap,
                              const double *rsold, const double *pAp, double *rr_out, const RedWs &ws, hipStream_t s,
                              const int64_t *gate, double eps, int64_t k, int64_t *kdone, double *rrfinal,
                              int64_t *hrec, int64_t *ts = nullptr);
hipError_t update_xp_f64(int64_t n, double *x, double *p, const double *r, const double *rsold, const double *pAp,
                         const double *rr, hipStream_t s, double eps = -1.0, int64_t k = 0,
                         int64_t *kdone = nullptr, double *rrfinal = nullptr, int64_t *hrec = nullptr,
                         int64_t *ts = nullptr, const PeerSum *rr_sum = nullptr);
hipError_t dot_f64(int64_t n, const double *a, const double *b, double *out,
                   const RedWs &ws, hipStream_t s);
// Rows [row0, row0+nrows) of the counter-hash SPD system; pad columns zeroed.
hipError_t gen_spd_f64(int64_t n, int64_t lda, int64_t row0, int64_t nrows, uint64_t seed,
                       double *A, double *b, hipStream_t s);
// CGX_A_F32: A_ij = (float) of gen_spd_f64's value (round to nearest), b as gen_spd_f64's.
hipError_t gen_spd_a32(int64_t n, int64_t lda, int64_t row0, int64_t nrows, uint64_t seed, float *A, double *b,
                       hipStream_t s);
// out = sum_{q<cnt} (8-byte slot q of in), in q order (one thread): rank-ordered combine.
hipError_t sum_ordered_f64(const double *in, int cnt, double *out, hipStream_t s);


// 5-point Poisson A.p on a slab of mloc grid rows of width m; ph has one halo
// row above and below.  *dot_out = ph[m..] . Ap when dot_out != nullptr.
hipError_t stencil5_f64(const double *ph, int64_t mloc, int64_t m, double *Ap, double *dot_out, const RedWs &ws,
                        hipStream_t s, const int64_t *gate = nullptr);
// Fused Poisson CG iteration (even m, 16-B-aligned buffers; see the kernels).
// rh, poh, pnh: r, p_{k-1}, p_k slabs with one halo row above and below.
bool poisson_fusable(int64_t mloc, int64_t m);
// part: 0 all rows; 1 interior runs; 2 the two edge runs (+= part 1's p.Ap).
// r_up / r_dn (one process, several slabs): r's top / bottom halo row is read
// in place from the neighbouring slab's boundary row (system-scope loads)
// instead of from rh's halo rows.  rr_sum: *rr is the rank-order sum of the
// slabs' r.r partials, formed by the kernel (block 0 stores it to rr_sum->out).
hipError_t poisson_p_f64(const double *rh, const double *poh, double *pnh, int64_t mloc, int64_t m, const double *rr,
                         const double *rsold, bool first, double *pap_out, const RedWs &ws, hipStream_t s,
                         double eps = -1.0, int64_t k = 0, int64_t *kdone = nullptr, double *rrfinal = nullptr,
                         int part = 0, int64_t *hrec = nullptr, const double *r_up = nullptr,
                         const double *r_dn = nullptr, const PeerSum *rr_sum = nullptr);
// xmode: 1 x += alpha p_k; 0 x untouched, alpha_k to *xalpha; 2 x += alpha_{k-1}
// p_{k-1} (poh, xalpha[0]) then += alpha_k p_k (x every other iteration);
// 3 x += alpha_{k-2} p_{k-2} (pqh, xalpha[0]), alpha_{k-1} p_{k-1} (poh,
// xalpha[1]), alpha_k p_k (x every third iteration).  pap_sum: p.Ap from the
// slabs' partials, as poisson_p_f64's rr_sum.
hipError_t poisson_xr_f64(const double *pnh, const double *poh, const double *pqh, double *x, double *r,
                          int64_t mloc, int64_t m, const double *rsold, const double *pAp, double *rr_out, int xmode,
                          double *xalpha, const RedWs &ws, hipStream_t s, const int64_t *gate = nullptr,
                          const PeerSum *pap_sum = nullptr);
// x += xalpha[0] p (pnh) [then += xalpha[1] p (pbh) when pbh != nullptr] over the
// slab interior: the x updates the last iterations left out.
hipError_t poisson_xflush_f64(const double *pnh, const double *pbh, double *x, int64_t mloc, int64_t m,
                              const double *xalpha, hipStream_t s);
hipError_t fill_f64(double *p, int64_t n, double v, hipStream_t s);
hipError_t fill_f32(float *p, int64_t n, float v, hipStream_t s);

// ---- CGX_SYMMETRIC: A as the upper triangle of 128 x 128 tiles ---------------
// (layout: cgx_symv.hip).  lda is a multiple of 128; At holds sym_tiles(lda)
// tiles of 128*128 doubles; prow 2*sym_tiles(lda)*128 doubles (one row
// partial per unit = half tile, at most), pcol sym_tiles(lda)*128.
int64_t sym_tiles(int64_t lda);
int sym_grid(int device);
// y = A p (rows [0, n)), *dot_out = pown . y when pown != nullptr
hipError_t symv_f64(const double *At, int64_t n, int64_t lda, int grid, const double *p, double *prow, double *pcol,
                    double *y, const double *pown, double *dot_out, const RedWs &ws, hipStream_t s,
                    const int64_t *gate = nullptr);
// rows [row0, row0+nrows) of A (row-major, leading dimension ld) into the tiles
hipError_t sym_pack_f64(const double *rows, int64_t ld, int64_t row0, int64_t nrows, int64_t n, int64_t lda,
                        double *At, hipStream_t s);
// the counter-hash SPD system of gen_spd_f64, packed; b for all n rows
hipError_t gen_spd_sym_f64(int64_t n, int64_t lda, uint64_t seed, double *At, double *b, hipStream_t s);
// Streamed pieces (CGX_SYMMETRIC | CGX_HOST_STREAM): tiles [q_base, q_base+count)
// held in At (At[0] = tile q_base).  tile_runs: row partials per tile (then
// reduce with per = 1).
hipError_t gen_spd_sym_tiles_f64(int64_t n, int64_t lda, uint64_t seed, int64_t q_base, int64_t count, double *At,
                                 hipStream_t s);
hipError_t gen_b_f64(int64_t n, uint64_t seed, double *b, hipStream_t s);
hipError_t symv_tiles_f64(const double *At, int64_t q_base, int64_t count, int64_t lda, int grid, bool tile_runs,
                          const double *p, double *prow, double *pcol, hipStream_t s, const int64_t *gate = nullptr);
hipError_t symv_reduce_f64(int64_t n, int64_t lda, int64_t per, const double *prow, const double *pcol, double *y,
                           const double *pown, double *dot_out, const RedWs &ws, hipStream_t s,
                           const int64_t *gate = nullptr);
// host copies of the layout helpers (tile index, element offset in a tile)
inline int64_t sym_off_h(int64_t I, int64_t nt) { return I * nt - I * (I - 1) / 2; }
inline int64_t sym_pos_h(int r, int c) {  // kSymNT = 256: unit c / 64, (8 tr + rr, 4 tc + 2 cc + e)
    const int h = c / 64, cc = c % 64;
    const int t = (r / 8) * 16 + (cc >> 2), k = (r % 8) * 2 + ((cc >> 1) & 1);
    return (int64_t)h * 128 * 64 + ((int64_t)k * 256 + t) * 2 + (c & 1);
}

// ---- fp32, serialConjugate.c operation order ---------------------------------
// gate: the device-side convergence record (kernels of an iteration after the
// converged one do nothing); update_p_ref_f32 with kdone makes the stopping
// decision (see k_update_p_ref_f32).
hipError_t matvec_ref_f32(const float *A, int64_t lda, int64_t rows, int64_t cols,
                          const float *v, float *out, hipStream_t s, const int64_t *gate = nullptr);
hipError_t dot_ref_f32(int64_t n, const float *a, const float *b, float *out, hipStream_t s,
                       const int64_t *gate = nullptr);
hipError_t residual_ref_f32(int64_t n, const float *b, const float *Ax, float *r, float *p,
                            hipStream_t s);
hipError_t update_xr_ref_f32(int64_t n, float *x, float *r, const float *p, const float *Ap,
                             const float *rsold, const float *pAp, hipStream_t s, const int64_t *gate = nullptr);
// one launch each: x += p alpha, r -= Ap alpha, *rr = r.r (serialConjugate.c:219-234) /
// r = p = b - Ax, *rr = r.r (:209-212); the same float operations as the separate kernels
// pap_sum (several row blocks in one process): p.Ap summed from the blocks'
// partials in MPICH order instead of read from *pAp, which block 0 stores.
hipError_t update_xr_dot_ref_f32(int64_t n, float *x, float *r, const float *p, const float *Ap, const float *rsold,
                                 const float *pAp, float *rr, hipStream_t s, const int64_t *gate = nullptr,
                                 const PeerSumF32 *pap_sum = nullptr);
hipError_t residual_dot_ref_f32(int64_t n, const float *b, const float *Ax, float *r, float *p, float *rr,
                                hipStream_t s, int64_t *clear2 = nullptr);  // clear2: as residual_f64
// The single-GPU two-launch F32_REF iteration (the same float operations as
// matvec_ref_f32 + dot_ref_f32 + update_xr_dot_ref_f32 + update_p_ref_f32):
// out = A v with *dot_out = pown . out from the matVec's last block (ticket:
// a zeroed counter), then x, r, *rr = r.r, the stopping decision and (unless
// stopped) p = r + p (*rr / *rsold) in one single-block launch.
bool matvec_dot_ref_f32_fusable(const float *A, int64_t lda, const float *v);
hipError_t matvec_dot_ref_f32(const float *A, int64_t lda, int64_t rows, int64_t cols, const float *v, float *out,
                              const float *pown, float *dot_out, unsigned *ticket, hipStream_t s,
                              const int64_t *gate = nullptr);
hipError_t update_xrp_dot_ref_f32(int64_t n, float *x, float *r, float *p, const float *Ap, const float *rsold,
                                  const float *pAp, float *rr, hipStream_t s, const int64_t *gate, double eps,
                                  int64_t k, int64_t *kdone, double *rrfinal, int64_t *hrec);
// rr_sum: likewise for r.r (stored to *rr by block 0)
hipError_t update_p_ref_f32(int64_t n, float *p, const float *r, const float *rr,
                            const float *rsold, hipStream_t s, double eps = -1.0, int64_t k = 0,
                            int64_t *kdone = nullptr, double *rrfinal = nullptr, int64_t *hrec = nullptr,
                            const PeerSumF32 *rr_sum = nullptr);
hipError_t gen_spd_f32(int64_t n, int64_t lda, int64_t row0, int64_t nrows, uint64_t seed,
                       float *A, float *b, hipStream_t s);
// F32_REF combine: rank order (allSum) or, with mpich, MPICH's MPI_Allreduce order.
hipError_t sum_ordered_f32(const float *in, int cnt, float *out, hipStream_t s, bool mpich);

// Each kernel file is its own code object, which HIP loads on a device at
// the first use of one of its kernels.  preload_kernels() loads the ones a
// context will launch from on the current device at context creation
// (overlapped with the CLI's file parsing), so no first launch inside a
// timed solve pays for a load.
hipError_t preload_matvec();
hipError_t preload_vector();
hipError_t preload_poisson();
hipError_t preload_ref_f32();
hipError_t preload_symv();
hipError_t preload_matvec_a32();
hipError_t preload_matvec_nrhs();
hipError_t preload_spmv();
hipError_t preload_spmm();
hipError_t preload_pcg();
hipError_t preload_pcg_block();
hipError_t preload_bsmv();
hipError_t preload_dia();
hipError_t preload_dia_sym();
enum PreloadSet : unsigned {
    PL_MATVEC = 1, PL_VECTOR = 2, PL_POISSON = 4, PL_REF_F32 = 8, PL_SYMV = 16, PL_MATVEC_A32 = 32,
    PL_MATVEC_NRHS = 64, PL_SPMV = 128, PL_PCG = 256, PL_SPMM = 512, PL_PCG_BLOCK = 1024, PL_BSMV = 2048,
    PL_DIA = 4096, PL_DIA_SYM = 8192
};
inline hipError_t preload_kernels(unsigned set) {
    const struct { unsigned bit; hipError_t (*fn)(); } all[] = {
        {PL_MATVEC, preload_matvec}, {PL_VECTOR, preload_vector}, {PL_POISSON, preload_poisson},
        {PL_REF_F32, preload_ref_f32}, {PL_SYMV, preload_symv}, {PL_MATVEC_A32, preload_matvec_a32},
        {PL_MATVEC_NRHS, preload_matvec_nrhs}, {PL_SPMV, preload_spmv}, {PL_PCG, preload_pcg},
        {PL_SPMM, preload_spmm}, {PL_PCG_BLOCK, preload_pcg_block}, {PL_BSMV, preload_bsmv},
        {PL_DIA, preload_dia}, {PL_DIA_SYM, preload_dia_sym}};
    for (const auto &e : all)
        if (set & e.bit) {
            const hipError_t r = e.fn();
            if (r != hipSuccess) return r;
        }
    return hipSuccess;
}

}  // namespace cgx
