// cgx_nrhs.hip -- cgx_create_nrhs contexts (cgx_ctx.h NrhsState): nrhs systems
// A x_j = b_j on one matrix, one read of A per iteration.
//
// The reference runs conjugrad (serialConjugate.c:180-259) once per
// vectorb.txt; K runs stream A K times per iteration.  Here the K recurrences
// run side by side -- batched CG, not block CG: each column has its own alpha,
// beta and stopping point -- and share k_matvec_nrhs_f64's one pass over A.
//
// The path is the context's own: begin, the three-launch iteration (matVec
// with the K fused p.Ap, r update with the K r.r, x / p update with the
// stopping decisions), the host loop and the data movers below.  The entry
// points of cgx_setup.hip and cgx_iterate.hip branch here at their top, so
// every other context's path is what it was.
//
// Freeze rule: the update kernel decides per column on the device; a stopped
// column keeps its x (with the stopping iteration's update), r, p and scalars
// from then on, whatever the other columns go on doing, so its result does
// not depend on its neighbours.  When the last column stops the kernel stores
// k+1 in NrhsScal::alldone (the gate of every later launch) and in the
// shard's host-mapped record, which the host loop reads one iteration behind
// (iterate_gated's lookahead, cgx_iterate.hip).
#include "cgx_ctx.h"

namespace cgxh {

static double *col(char *base, const cgx_ctx *c, int j) { return f64(base) + (size_t)j * c->lda; }

int nrhs_check_args(int nrhs, int flags, const char *fn) {
    if (nrhs < 1 || nrhs > CGX_MAX_NRHS)
        return fail(CGX_ERR_ARG, "%s: nrhs must be in [1, %d] (got %d)", fn, CGX_MAX_NRHS, nrhs);
    const struct {
        int bit;
        const char *name;
    } refused[] = {{CGX_F32_REF, "CGX_F32_REF"},         {CGX_A_F32, "CGX_A_F32"},
                   {CGX_SYMMETRIC, "CGX_SYMMETRIC"},     {CGX_HOST_STREAM, "CGX_HOST_STREAM"},
                   {CGX_PHASES, "CGX_PHASES"},           {CGX_COMM_P2P, "CGX_COMM_P2P"},
                   {CGX_NO_OVERLAP, "CGX_NO_OVERLAP"},   {CGX_DETERMINISTIC, "CGX_DETERMINISTIC"}};
    for (const auto &r : refused)
        if (flags & r.bit)
            return fail(CGX_ERR_ARG, "%s: CGX_F64 (optionally with CGX_TIMING) only, not %s", fn, r.name);
    if (flags & ~CGX_TIMING)
        return fail(CGX_ERR_ARG, "%s: CGX_F64 (optionally with CGX_TIMING) only (flags 0x%x)", fn, flags);
    return CGX_OK;
}

int nrhs_alloc(cgx_ctx *c, int nrhs) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    const size_t vb = (size_t)nrhs * (size_t)c->lda * 8;
    for (char **p : {&nr->b, &nr->x, &nr->r, &nr->p, &nr->Ap}) {
        hipError_t e = hipMalloc(p, vb);
        if (e != hipSuccess)
            return fail(CGX_ERR_NOMEM, "hipMalloc(%zu bytes) on device %d: %s", vb, s.dev, hipGetErrorString(e));
        HIPT(hipMemsetAsync(*p, 0, vb, s.stream));  // zero past n: p's tail is multiplied by A's zero padding
    }
    HIPT(hipMalloc(reinterpret_cast<void **>(&nr->sc), sizeof(NrhsScal)));
    HIPT(hipMemsetAsync(nr->sc, 0, sizeof(NrhsScal), s.stream));
    HIPT(hipHostMalloc(reinterpret_cast<void **>(&nr->h_sc), sizeof(NrhsScal), hipHostMallocDefault));
    std::memset(nr->h_sc, 0, sizeof(NrhsScal));
    HIPT(hipMalloc(reinterpret_cast<void **>(&nr->ws.partials), (size_t)kMaxNrhs * kMaxRedBlocks * sizeof(double)));
    HIPT(hipMalloc(reinterpret_cast<void **>(&nr->ws.tickets), kNrhsTickets * sizeof(unsigned)));
    HIPT(hipMemsetAsync(nr->ws.tickets, 0, kNrhsTickets * sizeof(unsigned), s.stream));
    const size_t xb = (size_t)nrhs * (size_t)c->n * 8;
    if (xb <= kXStageMax) HIPT(hipHostMalloc(reinterpret_cast<void **>(&nr->h_v), xb, hipHostMallocDefault));
    if (c->op == OP_CSR)  // cgx_set_csr plans again for the matrix it gets
        nr->plan = plan_spmm_csr(s.dev, s.nloc, c->csr_cap, nrhs_width(nrhs));
    else
        nr->plan = plan_matvec_nrhs(s.dev, s.nloc, nrhs_width(nrhs), 0, 0, -1, 0, c->lda);
    HIPT(hipStreamSynchronize(s.stream));
    return CGX_OK;
}

void nrhs_free(cgx_ctx *c) {
    NrhsState *nr = c->nr;
    if (!nr) return;
    if (!c->sh.empty()) {
        (void)hipSetDevice(c->sh[0].dev);
        if (c->sh[0].stream) (void)hipStreamSynchronize(c->sh[0].stream);
    }
    for (char *p : {nr->b, nr->x, nr->r, nr->p, nr->Ap})
        if (p) (void)hipFree(p);
    if (nr->sc) (void)hipFree(nr->sc);
    if (nr->h_sc) (void)hipHostFree(nr->h_sc);
    if (nr->ws.partials) (void)hipFree(nr->ws.partials);
    if (nr->ws.tickets) (void)hipFree(nr->ws.tickets);
    if (nr->h_v) (void)hipHostFree(nr->h_v);
    delete nr;
    c->nr = nullptr;
}

// b_rows / x_rows: nrhs blocks of nrows values, block j = rows [row0, row0+nrows) of system j.
int nrhs_set_vec_rows(cgx_ctx *c, int64_t row0, int64_t nrows, const void *b_rows, const void *x_rows) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    if (!b_rows && !x_rows) return CGX_OK;
    TRY(set_dev(s));
    for (int j = 0; j < nr->nrhs; ++j) {
        if (b_rows)
            HIPT(hipMemcpyAsync(col(nr->b, c, j) + row0, static_cast<const double *>(b_rows) + (size_t)j * nrows,
                                (size_t)nrows * 8, hipMemcpyHostToDevice, s.stream));
        if (x_rows)
            HIPT(hipMemcpyAsync(col(nr->x, c, j) + row0, static_cast<const double *>(x_rows) + (size_t)j * nrows,
                                (size_t)nrows * 8, hipMemcpyHostToDevice, s.stream));
    }
    if (x_rows) {
        bool zeros = true;  // +0 / -0 only (A x is then exactly zero)
        const double *xs = static_cast<const double *>(x_rows);
        for (int64_t i = 0; i < (int64_t)nr->nrhs * nrows && zeros; ++i) zeros = xs[i] == 0.0;
        const bool whole = row0 == 0 && nrows == c->n;
        nr->x_zero = whole ? zeros : (nr->x_zero && zeros);
        if (whole) c->x_incomplete = c->x_deferred = false;  // x fully defined again
    }
    HIPT(hipStreamSynchronize(s.stream));
    c->state = ST_IDLE;
    return CGX_OK;
}

int nrhs_get_x(cgx_ctx *c, void *x) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    char *dst = nr->h_v ? nr->h_v : static_cast<char *>(x);
    for (int j = 0; j < nr->nrhs; ++j)
        HIPT(hipMemcpyAsync(dst + (size_t)j * c->n * 8, col(nr->x, c, j), (size_t)c->n * 8, hipMemcpyDeviceToHost,
                            s.stream));
    HIPT(hipStreamSynchronize(s.stream));
    if (nr->h_v) std::memcpy(x, nr->h_v, (size_t)nr->nrhs * c->n * 8);
    return CGX_OK;
}

int nrhs_fill(cgx_ctx *c, double b_value, double x_value) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    for (int j = 0; j < nr->nrhs; ++j) {
        HIPT(fill_f64(col(nr->b, c, j), c->n, b_value, s.stream));
        HIPT(fill_f64(col(nr->x, c, j), c->n, x_value, s.stream));
    }
    nr->x_zero = x_value == 0.0;
    HIPT(hipStreamSynchronize(s.stream));
    c->state = ST_IDLE;
    return CGX_OK;
}

// b_j = the b of cgx_generate_spd(seed + j) (column 0: the one-system context's), x0 = 0
int nrhs_generate_b(cgx_ctx *c, uint64_t seed) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    for (int j = 0; j < nr->nrhs; ++j) {
        HIPT(gen_b_f64(c->n, seed + (uint64_t)j, col(nr->b, c, j), s.stream));
        HIPT(hipMemsetAsync(col(nr->x, c, j), 0, (size_t)c->n * 8, s.stream));
    }
    nr->x_zero = true;
    return CGX_OK;
}

// Out_j = A v_j for the context's columns (every column of A up to lda, as the
// one-system path runs them: A and the vectors are zero there); with_dot: the
// K fused p_j . Ap_j into the ring slot of iteration k.
static int nrhs_matvec(cgx_ctx *c, const char *vec, bool with_dot, int64_t k, bool gated) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(timing_begin(c, s));
    const double *pown = with_dot ? f64(vec) : nullptr;
    double *dots = with_dot ? &nr->sc->pap[ring(k)][0] : nullptr;
    const int64_t *gate = gated ? &nr->sc->alldone : nullptr;
    if (c->op == OP_CSR) {  // the indices were checked on the host before they were uploaded (cgx_set_csr)
        HIPT(spmm_csr_f64(nr->plan, reinterpret_cast<const int64_t *>(s.csr_rp),
                          reinterpret_cast<const int32_t *>(s.csr_ci), csr_values(c), s.nloc, nr->nrhs, f64(vec), c->lda,
                          f64(nr->Ap), c->lda, pown, c->lda, dots, nr->ws, s.stream, gate));
    } else {
        HIPT(matvec_nrhs_f64(nr->plan, f64(s.A), c->lda, s.nloc, c->lda, nr->nrhs, f64(vec), c->lda, f64(nr->Ap), c->lda,
                             pown, c->lda, dots, nr->ws, s.stream, gate));
    }
    TRY(timing_end(c, s));
    return CGX_OK;
}

// r_j = p_j = b_j - A x_j, r_j . r_j   (serialConjugate.c:209-212 per column);
// x0 = 0: A x0 is exactly zero, the matVec is skipped (do_begin's rule).
int nrhs_begin(cgx_ctx *c) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    // nothing of an earlier solve may still store its stopping record
    HIPT(hipStreamSynchronize(s.stream));
    s.h_rec[0] = s.h_rec[1] = 0;
    const bool zero = nr->x_zero;
    if (!zero) TRY(nrhs_matvec(c, nr->x, false, 0, false));
    nr->x_zero = false;  // the iterations update x
    HIPT(nrhs_residual_f64(c->n, c->lda, nr->nrhs, f64(nr->b), zero ? nullptr : f64(nr->Ap), f64(nr->r), f64(nr->p),
                           &nr->sc->rr[ring(0)][0], nr->sc, nullptr, nr->ws, s.stream));
    c->k = 0;
    c->converged = 0;
    c->state = ST_BEGUN;
    c->x_incomplete = c->x_deferred = false;
    c->iter_failed = false;
    return CGX_OK;
}

// Iteration k = c->k (serialConjugate.c:215-244 per column), three launches.
static int nrhs_iteration(cgx_ctx *c, double eps) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    const int64_t k = c->k;
    TRY(nrhs_matvec(c, nr->p, true, k, true));
    HIPT(nrhs_update_r_f64(c->n, c->lda, nr->nrhs, k, f64(nr->r), f64(nr->Ap), nr->sc, nr->ws, s.stream));
    HIPT(nrhs_update_xp_f64(c->n, c->lda, nr->nrhs, k, eps, f64(nr->x), f64(nr->p), f64(nr->r), nr->sc, s.d_rec,
                            s.stream));
    c->k = k + 1;
    c->total_iters += 1;
    return CGX_OK;
}

// The per-column outcome so far, read back after a sync: a stopped column's
// count and r.r from its record, a running column's from the context's count
// and the ring slot of the last iteration.
static int nrhs_refresh(cgx_ctx *c) {
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    HIPT(hipMemcpyAsync(nr->h_sc, nr->sc, sizeof(NrhsScal), hipMemcpyDeviceToHost, s.stream));
    HIPT(hipStreamSynchronize(s.stream));
    double worst = 0.0;
    for (int j = 0; j < nr->nrhs; ++j) {
        const int64_t kd = nr->h_sc->kdone[j];
        nr->iters[j] = kd ? kd : c->k;
        nr->conv[j] = kd != 0;
        nr->rr[j] = kd ? nr->h_sc->rrfinal[j] : nr->h_sc->rr[ring(c->k)][j];
        if (j == 0 || nr->rr[j] > worst || std::isnan(nr->rr[j])) worst = nr->rr[j];
    }
    if (c->state != ST_IDLE) c->last_rr = worst;
    return CGX_OK;
}

int nrhs_iterate(cgx_ctx *c, int64_t count, double eps, int64_t *done, int *converged) {
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    int64_t did = 0;
    volatile int64_t *rec = s.h_rec;  // alldone, stored by the update kernel that stopped the last column
    const int64_t k0 = c->k;
    if (c->state == ST_BEGUN && count > 0 && eps < 0.0) {
        // fixed count: nothing is decided, nothing is waited for
        for (; did < count; ++did) TRY(nrhs_iteration(c, eps));
    } else if (c->state == ST_BEGUN && count > 0) {
        const char *gv = std::getenv("CGX_GATED");
        const bool gated = !(gv && *gv == '0');
        const char *la = std::getenv("CGX_LOOKAHEAD");
        const int look = std::max(1, std::min(kLookRing - 1, (la && *la) ? std::atoi(la) : 1));
        int64_t issued = 0;
        for (; issued < count; ++issued) {
            if (rec[0] != 0) break;
            TRY(nrhs_iteration(c, eps));
            if (!gated) {  // CGX_GATED=0: the host looks after every iteration (the same kernels, the same bits)
                HIPT(hipStreamSynchronize(s.stream));
                continue;
            }
            HIPT(hipEventRecord(s.ev_look[issued % kLookRing], s.stream));
            if (issued >= look) HIPT(hipEventSynchronize(s.ev_look[(issued - look) % kLookRing]));
        }
        HIPT(hipStreamSynchronize(s.stream));
        const int64_t kdev = rec[0];
        did = kdev ? kdev - k0 : issued;
        c->total_iters += did - issued;  // nrhs_iteration counted every enqueued one
        c->k = k0 + did;
        if (kdev) {
            c->converged = 1;
            c->state = ST_CONVERGED;
        }
        TRY(nrhs_refresh(c));
    }
    if (done) *done = did;
    if (converged) *converged = c->converged;
    return CGX_OK;
}

int nrhs_solve(cgx_ctx *c, void *x_inout, double eps, int64_t max_iter, cgx_stats *st) {
    if (x_inout) TRY(cgx_set_x(c, x_inout));
    TRY(sync_all(c));
    const auto t0 = std::chrono::steady_clock::now();
    TRY(nrhs_begin(c));
    const int64_t cap = max_iter < 0 ? c->n : max_iter;  // for(k=0; k<ROWS; ++k)
    int64_t done = 0;
    int conv = 0;
    TRY(cgx_iterate(c, cap, eps, &done, &conv));
    TRY(sync_all(c));
    const auto t1 = std::chrono::steady_clock::now();
    c->solve_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (x_inout) TRY(cgx_get_x(c, x_inout));
    if (st) TRY(cgx_get_stats(c, st));
    return CGX_OK;
}

int nrhs_get_stats(cgx_ctx *c, cgx_stats *st) {
    NrhsState *nr = c->nr;
    TRY(sync_all(c));
    TRY(timing_resolve(c));
    TRY(nrhs_refresh(c));
    int64_t most = 0;
    int all = c->state != ST_IDLE || c->k > 0;
    for (int j = 0; j < nr->nrhs; ++j) {
        most = std::max(most, nr->iters[j]);
        all = all && nr->conv[j];
    }
    st->iterations = most;
    st->converged = all;
    st->rr = c->last_rr;
    st->solve_ms = c->solve_ms;
    st->matvec_ms = c->matvec_ms;
    st->matvec_count = c->matvec_count;
    st->total_iterations = c->total_iters;
    return CGX_OK;
}

int nrhs_set_plan(cgx_ctx *c, int R, int U, int nt, int blocks_per_cu) {
    NrhsState *nr = c->nr;
    const int K = nrhs_width(nr->nrhs);
    if (c->op == OP_CSR) {  // cgx_create_csr_nrhs: csr_set_plan's rule
        TRY(csr_plan_args(K, R, U, nt));
        TRY(set_dev(c->sh[0]));
        nr->plan = plan_spmm_csr(c->sh[0].dev, c->sh[0].nloc, c->csr_nnz >= 0 ? c->csr_nnz : c->csr_cap, K, 64 / R, nt,
                                 blocks_per_cu, c->csr_f32);
        c->csr_plan_user = true;
        return CGX_OK;
    }
    if (!matvec_nrhs_plan_ok(K, R, U, nt))
        return fail(CGX_ERR_ARG, "an nrhs context of width %d: (rows_per_wave, chunks_in_flight) must be one of %s and "
                                 "the load policy 2 or 8 (got %d, %d, %d)",
                    K, K == 2 ? "(2,4) (4,2) (4,4) (8,2)" : K == 4 ? "(4,2) (4,4) (8,2)" : "(4,1) (4,2)", R, U, nt);
    TRY(set_dev(c->sh[0]));
    nr->plan = plan_matvec_nrhs(c->sh[0].dev, c->sh[0].nloc, K, R, U, nt, blocks_per_cu, c->lda);
    return CGX_OK;
}

}  // namespace cgxh

extern "C" {

int cgx_get_nrhs(const cgx_ctx *c, int *nrhs) {
    if (!c || !nrhs) return fail(CGX_ERR_ARG, "NULL argument");
    *nrhs = c->nr ? c->nr->nrhs : 1;
    return CGX_OK;
}

int cgx_get_stats_rhs(cgx_ctx *c, int j, cgx_stats *st) {
    if (!c || !st) return fail(CGX_ERR_ARG, "NULL argument");
    const int nrhs = c->nr ? c->nr->nrhs : 1;
    if (j < 0 || j >= nrhs) return fail(CGX_ERR_ARG, "cgx_get_stats_rhs: system %d not in [0, %d)", j, nrhs);
    TRY(cgx_get_stats(c, st));
    if (c->nr) {
        st->iterations = c->nr->iters[j];
        st->converged = c->nr->conv[j];
        st->rr = c->nr->rr[j];
    }
    return CGX_OK;
}

int cgx_residual_norms(cgx_ctx *c, double *rnorm, double *bnorm) {
    const Range range_("cgx_residual_norms");
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    if (!c->nr) return cgx_residual_norm(c, rnorm, bnorm);
    TRY(csr_need_matrix(c, "cgx_residual_norms"));
    TRY(check_x_complete(c));
    NrhsState *nr = c->nr;
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    // ||b_j - A x_j|| with the current x: matVec, residual with its dot, b.b
    TRY(nrhs_matvec(c, nr->x, false, 0, false));
    HIPT(nrhs_residual_f64(c->n, c->lda, nr->nrhs, f64(nr->b), f64(nr->Ap), f64(nr->r), nullptr, &nr->sc->tr[0],
                           nullptr, nullptr, nr->ws, s.stream));
    HIPT(nrhs_dot_f64(c->n, c->lda, nr->nrhs, f64(nr->b), f64(nr->b), &nr->sc->tb[0], nr->ws, s.stream));
    HIPT(hipMemcpyAsync(nr->h_sc, nr->sc, sizeof(NrhsScal), hipMemcpyDeviceToHost, s.stream));
    HIPT(hipStreamSynchronize(s.stream));
    for (int j = 0; j < nr->nrhs; ++j) {
        if (rnorm) rnorm[j] = std::sqrt(nr->h_sc->tr[j]);
        if (bnorm) bnorm[j] = std::sqrt(nr->h_sc->tb[j]);
    }
    c->state = ST_IDLE;  // r was overwritten
    return CGX_OK;
}

int cgx_matvec_nrhs(const void *A, int64_t lda, int64_t rows, int64_t cols, int nrhs, const void *V, int64_t ldv,
                    void *Out, int64_t ldo, void *stream) {
    if (nrhs < 1 || nrhs > CGX_MAX_NRHS)
        return fail(CGX_ERR_ARG, "cgx_matvec_nrhs: nrhs must be in [1, %d] (got %d)", CGX_MAX_NRHS, nrhs);
    if (!A || !V || !Out) return fail(CGX_ERR_ARG, "cgx_matvec_nrhs: NULL pointer");
    if (rows < 0 || cols < 0 || lda < cols || (nrhs > 1 && (ldv < cols || ldo < rows)))
        return fail(CGX_ERR_SHAPE, "cgx_matvec_nrhs: bad shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double *Vd = static_cast<const double *>(V);
    double *Od = static_cast<double *>(Out);
    // An odd ldv leaves every other column of V off the 16-B grid while the
    // rest are on it: one launch cannot give both kinds cgx_matvec's order
    // (vector path / scalar tail), so the columns go one by one.
    if (nrhs > 1 && (ldv & 1) && (lda & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0) {
        for (int j = 0; j < nrhs; ++j) TRY(cgx_matvec(CGX_F64, A, lda, rows, cols, Vd + j * ldv, Od + j * ldo, stream));
        return CGX_OK;
    }
    int dev = 0;
    HIPT(hipGetDevice(&dev));
    const RedWs none{nullptr, nullptr};  // no fused dot: no reduction scratch
    HIPT(matvec_nrhs_f64(plan_matvec_nrhs(dev, rows, nrhs_width(nrhs), 0, 0, -1, 0, cols), static_cast<const double *>(A),
                         lda, rows, cols, nrhs, Vd, ldv, Od, ldo, nullptr, 0, nullptr, none, s));
    return CGX_OK;
}

}  // extern "C"
