// cgx_iterate.hip -- the conjugrad loop (cgx_ctx.h):
//   conjugrad()  serialConjugate.c:180-259 / parallel_cg.c:248-345
//     -> cgx_solve = cgx_solve_begin (:209-212) + cgx_iterate (:213-245)
// the matVec dispatch (resident, host-streamed, symmetric, Poisson), the
// iteration with its stopping test on the host or on the device (gating),
// and the true-residual check.
#include "cgx_ctx.h"

namespace cgxh {

// ---- the iteration pieces ----------------------------------------------------------
// One tile of the matVec: rows [r0, r0+rows) of this shard, A rows at `Arows`.
int matvec_rows(cgx_ctx *c, Shard &s, const MatvecPlan &pl, const char *Arows, int64_t r0, int64_t rows,
                const char *vec, bool fuse_dot, int dot_slot, bool gated, int64_t *ts) {
    if (f32ref(c)) {
        HIPT(matvec_ref_f32(f32(Arows), c->lda, rows, c->n, f32(vec), f32(s.Ap) + r0, s.stream, gate_of(s, gated)));
    } else if (a32(c)) {  // float A, fp64 everything else; every column to lda like the fp64 path
        HIPT(matvec_a32(pl, f32(Arows), c->lda, rows, c->lda, f64(vec), f64(s.Ap) + r0,
                        fuse_dot ? f64(s.pown) + r0 : nullptr, fuse_dot ? slot_f64(s, dot_slot) : nullptr, s.ws,
                        s.stream, gate_of(s, gated), ts));
    } else if (c->rot && Arows == s.A && r0 == 0 && rows == s.nloc) {
        // the block's own columns, then the rest, summed apart and added: the
        // overlapped form's bits in one launch (cgx_ctx::rot)
        HIPT(matvec_f64_cols(pl, f64(Arows), c->lda, rows, c->lda, s.row0, c->lda, false, f64(vec), f64(s.Ap),
                             fuse_dot ? f64(s.pown) : nullptr, fuse_dot ? slot_f64(s, dot_slot) : nullptr, s.ws,
                             s.stream, gate_of(s, gated), ts, s.nloc));
    } else {
        HIPT(matvec_f64(pl, f64(Arows), c->lda, rows, c->lda, f64(vec), f64(s.Ap) + r0,
                        fuse_dot ? f64(s.pown) + r0 : nullptr, fuse_dot ? slot_f64(s, dot_slot) : nullptr, s.ws,
                        s.stream, gate_of(s, gated), ts));
    }
    return CGX_OK;
}

// CGX_HOST_STREAM: the part of A that is not resident, `units` units of
// `unit_bytes` each at A_host (rows, or CGX_SYMMETRIC's tiles), from unit
// res_rows on in chunks of tile_rows.  Chunk t goes to buffer
// (next_buf++ % kStreamBufs); its copy waits until the kernel that last read
// that buffer is done (A is read-only, so copies of the next iteration's first
// chunks overlap this iteration's vector work); launch(buffer, first unit,
// count) enqueues its kernel on the compute stream, which waits for the copy.
template <class Launch>
static int stream_chunks(Shard &s, int64_t unit_bytes, int64_t units, Launch launch) {
    for (int64_t u0 = s.res_rows; u0 < units; u0 += s.tile_rows) {
        const int64_t cnt = std::min(s.tile_rows, units - u0);
        const int b = s.next_buf;
        s.next_buf = (s.next_buf + 1) % kStreamBufs;
        const int64_t bytes = cnt * unit_bytes;
        const char *src = s.A_host + (size_t)u0 * unit_bytes;
        const int64_t part = (bytes / s.ncopy + 4095) & ~int64_t(4095);
        for (int q = 0; q < s.ncopy; ++q) {
            const int64_t lo = std::min<int64_t>(bytes, q * part), hi = std::min<int64_t>(bytes, lo + part);
            if (s.buf_used[b]) HIPT(hipStreamWaitEvent(s.copy[q], s.ev_free[b], 0));
            if (hi > lo) HIPT(hipMemcpyAsync(s.tile[b] + lo, src + lo, hi - lo, hipMemcpyHostToDevice, s.copy[q]));
            HIPT(hipEventRecord(s.ev_loaded[b][q], s.copy[q]));
            HIPT(hipStreamWaitEvent(s.stream, s.ev_loaded[b][q], 0));
        }
        TRY(launch(s.tile[b], u0, cnt));
        HIPT(hipEventRecord(s.ev_free[b], s.stream));
        s.buf_used[b] = true;
    }
    return CGX_OK;
}

// CGX_HOST_STREAM matVec (stream_chunks).
// With resident rows (CGX_STREAM_RESIDENT_MB) their kernel goes first on the
// compute stream, so it runs while the copy streams bring in the first tiles
// of the rest (same row sums: every plan adds a row in the same order).
int matvec_streamed(cgx_ctx *c, Shard &s, const char *vec) {
    const int64_t row_bytes = c->lda * (int64_t)c->es;
    if (s.res_rows > 0) {
        if (s.res_dirty) {  // A changed on the host since the last copy (pinned: async)
            HIPT(hipMemcpyAsync(s.A, s.A_host, (size_t)s.res_rows * row_bytes, hipMemcpyHostToDevice, s.stream));
            s.res_dirty = false;
        }
        TRY(matvec_rows(c, s, s.res_plan, s.A, 0, s.res_rows, vec, false, 0));
    }
    return stream_chunks(s, row_bytes, s.nloc, [&](const char *tile, int64_t r0, int64_t rows) {
        return matvec_rows(c, s, s.tile_plan, tile, r0, rows, vec, false, 0);
    });
}

// CGX_SYMMETRIC | CGX_HOST_STREAM: the upper-triangle tiles stream from
// pinned host memory in chunks (stream_chunks, as matvec_streamed's rows);
// each chunk's k_symv_f64 writes per-tile row and column partials, and one
// reduce (with the fused p.Ap) follows the last chunk.
int matvec_sym_streamed(cgx_ctx *c, Shard &s, const char *vec, bool with_dot, int dot_slot, const int64_t *gate) {
    const int64_t ntiles = sym_tiles(c->lda), tb = 128 * 128 * 8;
    auto tiles = [&](const char *At, int64_t q0, int64_t cnt) {
        HIPT(symv_tiles_f64(f64(At), q0, cnt, c->lda, s.sym_grid, true, f64(vec), f64(s.sym_prow), f64(s.sym_pcol),
                            s.stream, gate));
        return (int)CGX_OK;
    };
    if (s.res_rows > 0) {  // the resident tiles first, under the copies of the rest (as matvec_streamed)
        if (s.res_dirty) {
            HIPT(hipMemcpyAsync(s.A, s.A_host, (size_t)s.res_rows * tb, hipMemcpyHostToDevice, s.stream));
            s.res_dirty = false;
        }
        TRY(tiles(s.A, 0, s.res_rows));
    }
    TRY(stream_chunks(s, tb, ntiles, tiles));
    HIPT(symv_reduce_f64(c->n, c->lda, 1, f64(s.sym_prow), f64(s.sym_pcol), f64(s.Ap),
                         with_dot ? f64(s.pown) : nullptr, with_dot ? slot_f64(s, dot_slot) : nullptr, s.ws, s.stream,
                         gate));
    return CGX_OK;
}

int launch_matvec(cgx_ctx *c, Shard &s, const char *vec, bool with_dot, int dot_slot, bool gated) {
    TRY(timing_begin(c, s));
    const bool streamed = (c->flags & CGX_HOST_STREAM) != 0;
    if (c->op == OP_CSR) {  // the same place in the iteration for every storage of the matrix
        const double *pown = with_dot ? f64(s.pown) : nullptr;
        double *dot = with_dot ? slot_f64(s, dot_slot) : nullptr;
        switch (c->storage) {
            case SK_DIA:
            case SK_DIA_SYM:  // the kind's diagonal kernel
                HIPT(dia_kind(c).spmv(s.plan, reinterpret_cast<const int32_t *>(s.csr_ci), f64(s.dia_data), c->dia_ld,
                                      s.nloc, c->dia_ndiag, f64(vec), f64(s.Ap), pown, dot, s.ws, s.stream,
                                      gate_of(s, gated), nullptr));
                break;
            case SK_BSR:  // the block kernel
                HIPT(spmv_bsr_f64(s.plan, c->bsr_bs, reinterpret_cast<const int64_t *>(s.csr_rp),
                                  reinterpret_cast<const int32_t *>(s.csr_ci), f64(s.bsr_val), s.nloc / c->bsr_bs,
                                  f64(vec), f64(s.Ap), pown, dot, s.ws, s.stream, gate_of(s, gated)));
                break;
            case SK_CSR:  // the indices were checked on the host before they were uploaded (cgx_set_csr)
                HIPT(spmv_csr_f64(s.plan, reinterpret_cast<const int64_t *>(s.csr_rp),
                                  reinterpret_cast<const int32_t *>(s.csr_ci), csr_values(c, s), s.nloc, f64(vec),
                                  f64(s.Ap), pown, dot, s.ws, s.stream, gate_of(s, gated)));
                break;
        }
    }
    else if (c->op == OP_POISSON)
        HIPT(stencil5_f64(f64(vec), s.nloc / c->m, c->m, f64(s.Ap), with_dot ? slot_f64(s, dot_slot) : nullptr, s.ws,
                          s.stream, gate_of(s, gated)));
    else if (streamed && (c->flags & CGX_SYMMETRIC))
        TRY(matvec_sym_streamed(c, s, vec, with_dot, dot_slot, gate_of(s, gated)));
    else if (streamed) TRY(matvec_streamed(c, s, vec));
    else if (c->flags & CGX_SYMMETRIC)
        HIPT(symv_f64(f64(s.A), c->n, c->lda, s.sym_grid, f64(vec), f64(s.sym_prow), f64(s.sym_pcol), f64(s.Ap),
                      with_dot ? f64(s.pown) : nullptr, with_dot ? slot_f64(s, dot_slot) : nullptr, s.ws, s.stream,
                      gate_of(s, gated)));
    else if (with_dot && c->ref_mv_dot)  // matVec + vecVec(p, Ap) in one launch (serialConjugate.c:215,219)
        HIPT(matvec_dot_ref_f32(f32(s.A), c->lda, s.nloc, c->n, f32(vec), f32(s.Ap), f32(s.pown),
                                slot_f32(s, dot_slot), s.ws.tickets + T_REF_MV, s.stream, gate_of(s, gated)));
    else TRY(matvec_rows(c, s, s.plan, s.A, 0, s.nloc, vec, with_dot && !f32ref(c), dot_slot, gated,
                         f32ref(c) ? nullptr : ts_of(c, s, TK_MV)));
    TRY(timing_end(c, s));
    if (with_dot && ((f32ref(c) && !c->ref_mv_dot) || (streamed && !(c->flags & CGX_SYMMETRIC)))) {
        if (f32ref(c))  // vecVec(p, Ap) sequential (serialConjugate.c:219)
            HIPT(dot_ref_f32(s.nloc, f32(s.pown), f32(s.Ap), slot_f32(s, dot_slot), s.stream, gate_of(s, gated)));
        else
            HIPT(dot_f64(s.nloc, f64(s.pown), f64(s.Ap), slot_f64(s, dot_slot), s.ws, s.stream));
    }
    return CGX_OK;
}

// Whether x0 is all zeros on every shard (every rank in rank mode: one
// int64 allreduce, so all ranks take the same branch of do_begin).
int x0_is_zero(cgx_ctx *c, bool *zero) {
    bool local = true;
    for (auto &s : c->sh) local = local && s.x_zero;
    if (c->mode != M_RCCL || c->nranks == 1) {
        *zero = local;
        return CGX_OK;
    }
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    int64_t *pin = reinterpret_cast<int64_t *>(s.h_pin);
    pin[0] = local ? 0 : 1;
    HIPT(hipMemcpyAsync(slot(s, S_XNZ), pin, 8, hipMemcpyHostToDevice, s.stream));
    NCCLC(c, ncclAllReduce(slot(s, S_XNZ), slot(s, S_XNZ), 1, ncclInt64, ncclSum, s.comm, s.stream),
          "ncclAllReduce(x0 != 0 count)");
    HIPT(hipMemcpyAsync(pin, slot(s, S_XNZ), 8, hipMemcpyDeviceToHost, s.stream));
    TRY(rank_wait_stream(c, s.stream, "the x0 check"));
    *zero = pin[0] == 0;
    return CGX_OK;
}

// The host's record of a solve at its start: do_begin's (ST_BEGUN), and what
// the creation warm-up goes back to (ST_IDLE, warm_solve_kernels).
// total_iters and last_rr outlive a solve and are not touched here.
static void reset_solve_state(cgx_ctx *c, State st) {
    for (auto &s : c->sh) s.h_rec[0] = s.h_rec[1] = 0;
    c->k = 0;
    c->converged = 0;
    c->state = st;
    c->x_incomplete = c->x_deferred = false;
    c->xalpha_pending = false;
    c->iter_failed = false;
}

int do_begin(cgx_ctx *c) {
    // r0 = p0 = b - A x0; rr0 = r0.r0   (serialConjugate.c:209-212, parallel_cg.c:283-287)
    // With x0 = 0 (the reference's usual initialguess, and the bench's) A x0 is
    // exactly zero for a finite A, so the exchange and the matVec are skipped:
    // r0 = b - 0 = b bit for bit, one matVec fewer per solve.  (An A holding
    // Inf or NaN gives NaN in A x0 at serialConjugate.c:209; cgx.h states the
    // finite-A precondition of the fp64 mode.)  CGX_F32_REF, the mode that
    // promises the reference's bits for any input, always does the matVec.
    TRY(settle_halo(c));
    bool zero = false;  // CGX_F32_REF always does the matVec: no need to ask (in rank mode: a collective)
    if (!f32ref(c)) TRY(x0_is_zero(c, &zero));
    // One GPU, CGX_F32_REF in HBM: the matVec reads x0 where it lies (its
    // vector loads stop at n, where pfull would be zero-padded), so x0 is not
    // copied into pfull first -- one copy fewer per solve.
    const bool x_direct = f32ref(c) && c->mode == M_SINGLE && !(c->flags & CGX_HOST_STREAM);
    if (!zero && !x_direct) TRY(exchange_allgather(c, /*from_x=*/true));  // full x0 into pfull
    // Poisson over several slabs of one process: exchange_halo put x0 into each slab's pown and the neighbours
    // copy their halo rows out of it on their own streams; the residual kernel below writes p0 into that pown.
    // Every stream waits for every slab's copies first.
    if (!zero && c->op == OP_POISSON && c->mode == M_LOCAL) TRY(local_barrier(c));
    const int gs = S_RR + ring(0), ls = S_LRR + ring(0);
    const int os = out_slot(c, ls, gs);
    for (auto &s : c->sh) {
        TRY(set_dev(s));
        if (!zero)
            TRY(launch_matvec(c, s, x_direct ? s.x : s.pfull, false, 0));
        s.x_zero = false;  // the iterations update x
        if (f32ref(c)) {
            HIPT(residual_dot_ref_f32(s.nloc, f32(s.b), f32(s.Ap), f32(s.r), f32(s.pown), slot_f32(s, os), s.stream,
                                      slot_i64(s, S_KDONE)));
        } else if (c->pc_kind == CGX_PC_BLOCK) {
            // block Jacobi: p0 = W r0 block by block, and r0.z0 beside r0.r0
            HIPT(pcgb_residual_f64(c->pc_bs, s.nloc, f64(s.b), zero ? nullptr : f64(s.Ap), f64(s.pc_w), s.pc_wld,
                                   f64(s.r), f64(s.pown), slot_f64(s, os), kRzStride, s.ws, s.stream,
                                   slot_i64(s, S_KDONE)));
        } else if (c->pc_kind != CGX_PC_NONE) {
            // preconditioned: p0 = minv o r0, and r0.z0 beside r0.r0 (one GPU: os is the global slot)
            HIPT(pcg_residual_f64(s.nloc, f64(s.b), zero ? nullptr : f64(s.Ap), f64(s.pc_minv), f64(s.r), f64(s.pown),
                                  slot_f64(s, os), kRzStride, s.ws, s.stream, slot_i64(s, S_KDONE)));
        } else {
            // x0 = 0: Ax = nullptr (r = b - 0.0, no Ap buffer to clear); the
            // kernel also resets the convergence record (no memset launch)
            HIPT(residual_f64(s.nloc, f64(s.b), zero ? nullptr : f64(s.Ap), f64(s.r), f64(s.pown), slot_f64(s, os), s.ws,
                              s.stream, slot_i64(s, S_KDONE)));
        }
    }
    TRY(exchange_scalar(c, ls, gs));
    c->rr_unsummed = false;
    // r0's halo rows for k_poisson_p (which reads them in place itself with halo_pull)
    if (c->fused && !c->halo_pull) TRY(exchange_halo_of(c, &Shard::rh));
    // The device-side convergence record {kdone, r.r} was reset by the residual
    // kernel above (k_residual_f64 / k_dot_ref_f32_blk<kDotResid>); the host copy here.
    reset_solve_state(c, ST_BEGUN);  // no kernel of this solve has run yet (do_begin follows a sync)
    return CGX_OK;
}

int read_scalar(cgx_ctx *c, int gslot, double *out) {
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    HIPT(hipMemcpyAsync(s.h_pin, slot(s, gslot), 8, hipMemcpyDeviceToHost, s.stream));
    TRY(rank_wait_stream(c, s.stream, "a scalar read-back"));
    if (f32ref(c)) {
        float f;
        std::memcpy(&f, s.h_pin, 4);
        *out = (double)f;
    } else {
        *out = s.h_pin[0];
    }
    return CGX_OK;
}

// The host-checked stop after iteration c->k - 1, whose r.r is in slot rg:
// if (sqrt(beta) < EPSILON) break;  serialConjugate.c:235-238.  eps < 0
// (fixed count): nothing is read back.
static int host_check_stop(cgx_ctx *c, int rg, double eps, int *stop) {
    if (eps < 0.0) return CGX_OK;
    double rr = 0.0;
    TRY(read_scalar(c, rg, &rr));
    c->last_rr = rr;
    if (std::sqrt(rr) < eps) {
        c->converged = 1;
        c->state = ST_CONVERGED;
        *stop = 1;
    }
    return CGX_OK;
}

// Fused Poisson iteration k (conjgrad.m's loop, two kernels, 64 B per grid
// point; see k_poisson_p_f64 / k_poisson_xr_f64):
//   p_k = r_k + beta p_{k-1}, p_k . A p_k      (gated: first decides the
//                                               previous iteration's stop)
//   allreduce(p.Ap)
//   x += alpha p_k, r -= alpha A p_k, r.r
//   allreduce(r.r); host-checked stop; r's halo rows for the next iteration.
// x is updated every c->xd-th iteration (c->xd > 1: a left-out iteration's
// alpha is kept in S_XALPHA + j and its p_k stays in its slab until the
// catching-up xr kernel has read it); poisson_x_finish completes it at the end
// of a cgx_iterate call.
// Where p_k lives: two slabs alternate (pfull for even k), three rotate with x every third iteration.
static char *poisson_slab(const cgx_ctx *c, const Shard &s, int64_t k) {
    if (c->xd == 3) {
        const int64_t q = ((k % 3) + 3) % 3;
        return q == 0 ? s.pfull : q == 1 ? s.p2 : s.p3;
    }
    return (k & 1) ? s.p2 : s.pfull;
}

int do_iteration_poisson(cgx_ctx *c, double eps, int *stop, bool gated) {
    const int64_t k = c->k;
    *stop = 0;
    const int64_t m = c->m;
    const int pg = S_PAP + ring(k), pl = S_LPAP + ring(k);
    const int rk = S_RR + ring(k), rkm1 = S_RR + ring(k + 3);  // r.r of iterations k, k-1
    const bool split = c->halo_pending;  // interior runs while the r halo exchange is in flight
    // x every D-th iteration (D = c->xd): leave it out at the first D-1 of every
    // D iterations from k0 (alpha_k to slot S_XALPHA + j), catch up at the D-th
    const int64_t jx = (k - c->xd_k0) % c->xd;
    const int xmode = c->xd == 1 ? 1 : jx == c->xd - 1 ? c->xd : 0;
    const int xslot = S_XALPHA + (xmode == 0 ? (int)jx : 0);
    // One process, several slabs (c->fuse_combine): the scalar combines are
    // folded into the kernels that consume them -- p.Ap into k_poisson_xr,
    // r.r into the next k_poisson_p (not when the host reads r.r after the
    // iteration: then a combine kernel forms it) -- and r's halo rows are read
    // in place from the neighbouring slabs by k_poisson_p (c->halo_pull).
    // Both wait on the same cross-stream events the combines waited on.
    const bool fold_rr = c->fuse_combine && (gated || eps < 0.0);
    const int S = (int)c->sh.size();
    const int64_t mloc = c->sh[0].nloc / m;
    for (int q = 0; q < S; ++q) {
        Shard &s = c->sh[q];
        TRY(set_dev(s));
        char *pold = poisson_slab(c, s, k - 1), *pnew = poisson_slab(c, s, k);
        // the previous slab's last interior row of r, the next slab's first
        const double *r_up = c->halo_pull && q > 0 ? f64(c->sh[q - 1].rh) + mloc * m : nullptr;
        const double *r_dn = c->halo_pull && q < S - 1 ? f64(c->sh[q + 1].r) : nullptr;
        const PeerSum rs = c->rr_unsummed ? peer_sum(c, s, S_LRR + ring(k), rk) : PeerSum{};
        for (int part : split ? std::initializer_list<int>{1, 2} : std::initializer_list<int>{0}) {
            if (part == 2) HIPT(hipStreamWaitEvent(s.stream, s.ev_gathered, 0));
            HIPT(poisson_p_f64(f64(s.rh), f64(pold), f64(pnew), mloc, m, slot_f64(s, rk), slot_f64(s, rkm1), k == 0,
                               slot_f64(s, out_slot(c, pl, pg)), s.ws, s.stream, gated ? eps : -1.0, k,
                               gated ? slot_i64(s, S_KDONE) : nullptr, gated ? slot_f64(s, S_RRFINAL) : nullptr, part,
                               rec_of(c, s, gated), r_up, r_dn, c->rr_unsummed ? &rs : nullptr));
        }
    }
    c->rr_unsummed = false;
    c->halo_pending = false;
    if (c->fuse_combine) TRY(local_barrier(c));  // MPI_Allreduce(p.Ap): summed by k_poisson_xr itself
    else TRY(exchange_scalar(c, pl, pg));
    const int rg = S_RR + ring(k + 1), rl = S_LRR + ring(k + 1);
    const int ro = out_slot(c, rl, rg);
    for (auto &s : c->sh) {
        TRY(set_dev(s));
        TRY(timing_begin(c, s));
        char *pnew = poisson_slab(c, s, k), *pold = poisson_slab(c, s, k - 1),
             *pq = c->xd == 3 ? poisson_slab(c, s, k - 2) : nullptr;
        const PeerSum ps = c->fuse_combine ? peer_sum(c, s, pl, pg) : PeerSum{};
        HIPT(poisson_xr_f64(f64(pnew), f64(pold), f64(pq), f64(s.x), f64(s.r), mloc, m, slot_f64(s, rk),
                            slot_f64(s, pg), slot_f64(s, ro), xmode, slot_f64(s, xslot), s.ws, s.stream,
                            gate_of(s, gated), c->fuse_combine ? &ps : nullptr));
        TRY(timing_end(c, s));
    }
    c->xalpha_pending = xmode == 0;  // the catch-up (xmode xd) and every-iteration x (1) leave nothing out
    if (fold_rr) {  // MPI_Allreduce(r.r): summed by the next k_poisson_p (or settle_rr)
        TRY(local_barrier(c));
        c->rr_unsummed = true;
    } else {
        TRY(exchange_scalar(c, rl, rg));
    }
    c->k = k + 1;
    c->total_iters += 1;
    if (!gated) TRY(host_check_stop(c, rg, eps, stop));
    if (*stop) return CGX_OK;  // before the halo exchange: no next iteration reads r
    if (c->halo_pull) return CGX_OK;  // the next k_poisson_p reads the neighbours' rows itself
    return c->halo_overlap ? exchange_halo_async(c) : exchange_halo_of(c, &Shard::rh);
}

// The r.r of the last iteration enqueued, when its combine was left to the
// next k_poisson_p (rr_unsummed): formed now by the combine kernels, for the
// host to read (or a later call's first k_poisson_p, which sums the same
// partials again).
int settle_rr(cgx_ctx *c) {
    if (!c->rr_unsummed) return CGX_OK;
    TRY(exchange_scalar(c, S_LRR + ring(c->k), S_RR + ring(c->k)));
    c->rr_unsummed = false;
    return CGX_OK;
}

// The end of a cgx_iterate call (the device's loop count known: c->k): when
// the last iteration run left x's update out (xmode 0), x += alpha_K p_K.
// Gated solves enqueue iterations past the stop that skip themselves, so this
// is decided from c->k, never from what was enqueued.
int poisson_x_finish(cgx_ctx *c) {
    if (!c->fused || c->xd == 1) return CGX_OK;
    const int64_t last = c->k - 1;
    const int64_t jx = last >= c->xd_k0 ? (last - c->xd_k0) % c->xd : c->xd - 1;
    if (jx != c->xd - 1) {  // jx + 1 updates left out: iterations last - jx .. last
        for (auto &s : c->sh) {
            TRY(set_dev(s));
            char *pa = poisson_slab(c, s, last - jx), *pb = jx == 1 ? poisson_slab(c, s, last) : nullptr;
            HIPT(poisson_xflush_f64(reinterpret_cast<const double *>(pa), reinterpret_cast<const double *>(pb),
                                    reinterpret_cast<double *>(s.x), s.nloc / c->m, c->m,
                                    reinterpret_cast<const double *>(slot(s, S_XALPHA)), s.stream));
        }
    }
    c->xd_k0 = c->k;
    c->xalpha_pending = false;
    return CGX_OK;
}

int check_x_complete(const cgx_ctx *c) {
    if (!c->x_incomplete) return CGX_OK;
    if (c->x_deferred)
        return fail(CGX_ERR_STATE, "an earlier cgx_iterate failed with x updates still deferred (Poisson, x every "
                                   "%d-th iteration): x is incomplete until cgx_set_x or the next cgx_solve_begin",
                    c->xd);
    return fail(CGX_ERR_STATE, "an earlier cgx_iterate failed part-way through iteration %lld: x may hold part of it "
                               "and is incomplete until cgx_set_x or the next cgx_solve_begin", (long long)c->k);
}

// ---- one GPU, two launches per iteration --------------------------------------------
// Each form below is its matVec launch and its update launch, with p.Ap in
// slot pg and the new r.r in slot rg; do_iteration_two_launch is the frame
// they share.
//
// A small dense fp64 system (c->fused_p): the matVec with its fused p.Ap, then
// k_update_xrp_f64, whose last block decides the stop and forms p for the next
// iteration.  The same expressions in the same order as do_iteration's three
// launches (bitwise the same x), one kernel boundary and one host launch fewer
// per iteration.
static int launch_fused_p(cgx_ctx *c, Shard &s, int64_t k, int pg, int rg, double eps, bool gated) {
    TRY(launch_matvec(c, s, s.pfull, true, pg, gated));  // serialConjugate.c:215,219
    HIPT(update_xrp_f64(s.nloc, f64(s.x), f64(s.r), f64(s.pown), f64(s.Ap), slot_f64(s, S_RR + ring(k)),
                        slot_f64(s, pg), slot_f64(s, rg), s.ws, s.stream, gate_of(s, gated), gated ? eps : -1.0, k,
                        gated ? slot_i64(s, S_KDONE) : nullptr, gated ? slot_f64(s, S_RRFINAL) : nullptr,
                        rec_of(c, s, gated), ts_of(c, s, TK_UXP)));  // :221-243
    return CGX_OK;
}

// ... with the p update folded into the matVec (c->fold_p):
// k_matvec_fold_f64 forms p_k = r_k + beta p_{k-1} as it
// multiplies it (its row owners store p_k into the other p buffer and fuse
// p_k . A p_k), then k_update_xr_stop_f64 does x, r, r.r and the stopping
// decision on every block -- no single-block pass over p.  Iteration 0 uses
// p_0 = r_0 as the residual left it.  p_k lives in pfull for even k, in
// p_alt for odd k.  The expressions are the three-launch kernels' (bitwise
// the same x, test_two_launch_iteration_bitwise_equals_three).
static int launch_fold_p(cgx_ctx *c, Shard &s, int64_t k, int pg, int rg, double eps, bool gated) {
    char *pk = (k & 1) ? s.p_alt : s.pfull, *pkm1 = (k & 1) ? s.pfull : s.p_alt;
    if (k == 0) {
        TRY(launch_matvec(c, s, s.pfull, true, pg, gated));  // serialConjugate.c:215,219 with p_0 = r_0
    } else {
        TRY(timing_begin(c, s));
        // every column up to lda, as the plain matVec runs them (A, r and both p
        // buffers are zero there), so the row sums add in the same order
        HIPT(matvec_fold_f64(s.fold_plan, f64(s.A), c->lda, s.nloc, c->lda, f64(s.r), f64(pkm1), f64(pk),
                             slot_f64(s, S_RR + ring(k)), slot_f64(s, S_RR + ring(k + 3)), f64(s.Ap), slot_f64(s, pg),
                             s.ws, s.stream, gate_of(s, gated), ts_of(c, s, TK_MV)));  // :239-243 of k-1, then :215,219
        TRY(timing_end(c, s));
    }
    HIPT(update_xr_stop_f64(s.nloc, f64(s.x), f64(s.r), f64(pk), f64(s.Ap), slot_f64(s, S_RR + ring(k)),
                            slot_f64(s, pg), slot_f64(s, rg), s.ws, s.stream, gate_of(s, gated), gated ? eps : -1.0,
                            k, gated ? slot_i64(s, S_KDONE) : nullptr, gated ? slot_f64(s, S_RRFINAL) : nullptr,
                            rec_of(c, s, gated), ts_of(c, s, TK_UXP)));
    return CGX_OK;
}

// The same for CGX_F32_REF (c->ref_fused): the matVec whose last block runs
// vecVec(p, Ap), then one single-block launch for x += p alpha, r -= Ap alpha,
// r.r, the stopping test and p = r + p (rr/rsold) -- four launches' float
// operations in their order (bitwise the same x and loop count).
static int launch_ref_fused(cgx_ctx *c, Shard &s, int64_t k, int pg, int rg, double eps, bool gated) {
    TRY(launch_matvec(c, s, s.pfull, true, pg, gated));  // serialConjugate.c:215,219
    HIPT(update_xrp_dot_ref_f32(s.nloc, f32(s.x), f32(s.r), f32(s.pown), f32(s.Ap), slot_f32(s, S_RR + ring(k)),
                                slot_f32(s, pg), slot_f32(s, rg), s.stream, gate_of(s, gated), gated ? eps : -1.0, k,
                                gated ? slot_i64(s, S_KDONE) : nullptr, gated ? slot_f64(s, S_RRFINAL) : nullptr,
                                rec_of(c, s, gated)));  // :220-243
    return CGX_OK;
}

static int do_iteration_two_launch(cgx_ctx *c, double eps, int *stop, bool gated) {
    const int64_t k = c->k;
    *stop = 0;
    Shard &s = c->sh[0];
    const int pg = S_PAP + ring(k), rg = S_RR + ring(k + 1);
    const bool phases = !c->ref_fused;  // the F32_REF kernels stamp no phases
    if (phases) TRY(phase_iter_begin(c));
    if (c->fold_p) TRY(launch_fold_p(c, s, k, pg, rg, eps, gated));
    else if (c->fused_p) TRY(launch_fused_p(c, s, k, pg, rg, eps, gated));
    else TRY(launch_ref_fused(c, s, k, pg, rg, eps, gated));
    if (phases) phase_iter_end(c);
    c->k = k + 1;
    c->total_iters += 1;
    if (!gated) TRY(host_check_stop(c, rg, eps, stop));  // x is already current
    return CGX_OK;
}

// ---- the row blocks' update launches ---------------------------------------------------
// Row block s, iteration k, after the p.Ap combine (or its barrier, when the
// kernel sums the partials itself: fuse_combine / fuse_f32).
int launch_update_r(const cgx_ctx *c, const Shard &s, int64_t k, bool gated) {
    const int pg = S_PAP + ring(k), pl = S_LPAP + ring(k), rk = S_RR + ring(k);
    const int ro = out_slot(c, S_LRR + ring(k + 1), S_RR + ring(k + 1));
    if (f32ref(c)) {
        // x += alpha p; r -= alpha Ap; r.r in one launch  (serialConjugate.c:219-234)
        const PeerSumF32 ps = c->fuse_f32 ? peer_sum_f32(c, s, pl, pg) : PeerSumF32{};
        HIPT(update_xr_dot_ref_f32(s.nloc, f32(s.x), f32(s.r), f32(s.pown), f32(s.Ap), slot_f32(s, rk),
                                   slot_f32(s, pg), slot_f32(s, ro), s.stream, gate_of(s, gated),
                                   c->fuse_f32 ? &ps : nullptr));
    } else if (c->pc_kind == CGX_PC_BLOCK) {
        // r -= alpha Ap with alpha = r.z / p.Ap; z = W r stored; r.r and r.z from the one pass
        HIPT(pcgb_update_r_f64(c->pc_bs, s.nloc, f64(s.r), f64(s.Ap), f64(s.pc_w), s.pc_wld, f64(s.pc_z),
                               slot_f64(s, rk + kRzStride), slot_f64(s, pg), slot_f64(s, ro), kRzStride, s.ws,
                               s.stream, gate_of(s, gated)));
    } else if (c->pc_kind != CGX_PC_NONE) {
        // r -= alpha Ap with alpha = r.z / p.Ap; r.r and r.z (z = minv o r) from the one pass
        HIPT(pcg_update_r_f64(s.nloc, f64(s.r), f64(s.Ap), f64(s.pc_minv), slot_f64(s, rk + kRzStride), slot_f64(s, pg),
                              slot_f64(s, ro), kRzStride, s.ws, s.stream, gate_of(s, gated)));
    } else {
        // r -= alpha Ap, r.r; x's update is deferred into the p update
        const PeerSum ps = c->fuse_combine ? peer_sum(c, s, pl, pg) : PeerSum{};
        HIPT(update_r_f64(s.nloc, f64(s.r), f64(s.Ap), slot_f64(s, rk), slot_f64(s, pg), slot_f64(s, ro), s.ws,
                          s.stream, gate_of(s, gated), ts_of(c, s, TK_UR), c->fuse_combine ? &ps : nullptr));
    }
    return CGX_OK;
}

// ... and after the r.r combine (fold_rr: after its barrier, the kernel sums
// the partials): p = r + (beta/rsold) p  (serialConjugate.c:239-243), in fp64
// after the x += alpha p deferred from the r update.  Only a deciding kernel
// (XP_DECIDE) gets the stop arguments; XP_X_ONLY passes no r.r, so the kernel
// leaves p alone (F32_REF: nothing to launch, x is current).
int launch_update_xp(const cgx_ctx *c, const Shard &s, int64_t k, XpForm form, double eps, bool fold_rr) {
    const int pg = S_PAP + ring(k), rk = S_RR + ring(k);
    const int rg = S_RR + ring(k + 1), rl = S_LRR + ring(k + 1);
    const bool decide = form == XP_DECIDE;
    const double stop_eps = decide ? eps : -1.0;
    const int64_t stop_k = decide ? k : 0;
    int64_t *kdone = decide ? slot_i64(s, S_KDONE) : nullptr;
    double *rrfinal = decide ? slot_f64(s, S_RRFINAL) : nullptr;
    if (f32ref(c)) {
        if (form == XP_X_ONLY) return CGX_OK;
        const PeerSumF32 ps = fold_rr ? peer_sum_f32(c, s, rl, rg) : PeerSumF32{};
        HIPT(update_p_ref_f32(s.nloc, f32(s.pown), f32(s.r), slot_f32(s, rg), slot_f32(s, rk), s.stream, stop_eps,
                              stop_k, kdone, rrfinal, rec_of(c, s, decide), fold_rr ? &ps : nullptr));
    } else if (c->pc_kind == CGX_PC_BLOCK) {
        // x += alpha p; p = z + (r.z_new / r.z_old) p with the z the r update stored; the stop as below
        HIPT(pcgb_update_xp_f64(s.nloc, f64(s.x), f64(s.pown), f64(s.pc_z), slot_f64(s, rk + kRzStride),
                                slot_f64(s, pg), form == XP_X_ONLY ? nullptr : slot_f64(s, rg),
                                slot_f64(s, rg + kRzStride), s.stream, stop_eps, stop_k, kdone, rrfinal,
                                rec_of(c, s, decide)));
    } else if (c->pc_kind != CGX_PC_NONE) {
        // x += alpha p; p = minv o r + (r.z_new / r.z_old) p; the stop is decided on r.r as below
        HIPT(pcg_update_xp_f64(s.nloc, f64(s.x), f64(s.pown), f64(s.r), f64(s.pc_minv), slot_f64(s, rk + kRzStride),
                               slot_f64(s, pg), form == XP_X_ONLY ? nullptr : slot_f64(s, rg),
                               slot_f64(s, rg + kRzStride), s.stream, stop_eps, stop_k, kdone, rrfinal,
                               rec_of(c, s, decide)));
    } else {
        const PeerSum ps = fold_rr ? peer_sum(c, s, rl, rg) : PeerSum{};
        HIPT(update_xp_f64(s.nloc, f64(s.x), f64(s.pown), f64(s.r), slot_f64(s, rk), slot_f64(s, pg),
                           form == XP_X_ONLY ? nullptr : slot_f64(s, rg), s.stream, stop_eps, stop_k, kdone, rrfinal,
                           rec_of(c, s, decide), ts_of(c, s, TK_UXP), fold_rr ? &ps : nullptr));
    }
    return CGX_OK;
}

// One loop iteration k (serialConjugate.c:215-244 / parallel_cg.c:290-323).
// Returns 1 in *stop when sqrt(r.r) < eps ended the loop (before the p update,
// as the reference breaks at :235-238).
// gated: fp64 device-side convergence (the host does not read r.r here; the
// update kernel decides sqrt(r.r) < eps and later kernels skip themselves).
int do_iteration(cgx_ctx *c, double eps, int *stop, bool gated) {
    if (c->fused) return do_iteration_poisson(c, eps, stop, gated);
    if (c->fold_p || c->fused_p || c->ref_fused) return do_iteration_two_launch(c, eps, stop, gated);
    const int64_t k = c->k;
    *stop = 0;
    const int pg = S_PAP + ring(k), pl = S_LPAP + ring(k);
    TRY(phase_iter_begin(c));
    if (c->pool && (gated || eps < 0.0)) {  // each row block's thread enqueues its own work (cgx_local_mt.hip)
        TRY(local_mt_iteration(c, eps, gated));
        phase_iter_end(c);
        c->k = k + 1;
        c->total_iters += 1;
        return CGX_OK;
    }
    if (c->overlap) {
        TRY(overlapped_matvec(c, out_slot(c, pl, pg), gated));  // parallel_cg.c:290-293, overlapped
    } else {
        TRY(exchange_allgather(c, false));  // MPI_Allgather(local_p -> p)  parallel_cg.c:290
        for (auto &s : c->sh) {
            TRY(set_dev(s));
            TRY(launch_matvec(c, s, s.pfull, true, out_slot(c, pl, pg), gated));  // :215 / :292-293
        }
    }
    // MPI_Allreduce(p.Ap)  parallel_cg.c:294 -- multi-shard fp64: summed by
    // k_update_r_f64 itself after the barrier (fuse_combine)
    // (F32_REF, fuse_f32: summed in MPICH order by k_dot_ref_f32_blk<kDotXR>)
    const bool fold = c->fuse_combine || c->fuse_f32;
    if (fold) TRY(local_barrier(c));
    else TRY(exchange_scalar(c, pl, pg));
    for (auto &s : c->sh) {
        TRY(set_dev(s));
        TRY(launch_update_r(c, s, k, gated));
    }
    const int rg = S_RR + ring(k + 1), rl = S_LRR + ring(k + 1);
    // the r.r combine folds into k_update_xp_f64 (F32_REF: k_update_p_ref_f32)
    // unless the host reads r.r first (host-checked convergence)
    const bool fuse_rr = fold && (gated || eps < 0.0);
    if (fuse_rr) TRY(local_barrier(c));  // MPI_Allreduce(r.r)  parallel_cg.c:313, summed by k_update_xp_f64
    else TRY(exchange_scalar(c, rl, rg));
    c->k = k + 1;
    c->total_iters += 1;
    if (!gated) TRY(host_check_stop(c, rg, eps, stop));
    // gated: x (+ p unless converged) on the device, stopping rule decided
    // there; a stop the host saw: the deferred x += alpha p, without the p
    // update (F32_REF: x is current, nothing more to enqueue)
    const XpForm form = gated ? XP_DECIDE : *stop ? XP_X_ONLY : XP_UPDATE;
    if (!(form == XP_X_ONLY && f32ref(c)))
        for (auto &s : c->sh) {
            TRY(set_dev(s));
            TRY(launch_update_xp(c, s, k, form, eps, fuse_rr));
        }
    phase_iter_end(c);
    return CGX_OK;
}

// The first launch of each kernel in a process costs the HIP runtime several
// microseconds more than later launches (rocprofv3 --hip-trace of a fresh
// process's first solve: 9-14 us against 6-7 us per hipLaunchKernel), about
// 20 us over a small system's first solve -- the only solve `cg_hip` runs.
// One GPU, small n: the context pays it at creation.  The solve's start runs
// for real on alloc_shard's zeroed x and b (A x with x = 0, whatever A holds),
// then two gated iterations whose kernels all return at once (the record
// holds -1: converged before any iteration, under both gate tests) and one
// record of each lookahead event; the written buffers and the host state then
// go back to what alloc_shard left.  CGX_WARM=0: no warm-up.
// What that can write on an eligible context -- one GPU, dense, A resident
// and not symmetric (no tile buffers, no symv partials), no timing events, no
// phase stamps -- and so what warm_solve_kernels clears: r, Ap, pfull, p_alt
// (the folded form's) and the scalar slots.
constexpr int64_t kWarmMaxN = 16384;
bool warm_eligible(const cgx_ctx *c) {
    if (c->mode != M_SINGLE || c->op != OP_DENSE || c->n > kWarmMaxN) return false;
    if (c->nr) return false;  // an nrhs context's buffers are not on warm_solve_kernels' restore list
    if (c->flags & (CGX_TIMING | CGX_PHASES | CGX_HOST_STREAM | CGX_SYMMETRIC)) return false;
    const char *e = std::getenv("CGX_WARM");
    return !(e && *e == '0');
}

int warm_solve_kernels(cgx_ctx *c) {
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    TRY(do_begin(c));
    int64_t *pin = reinterpret_cast<int64_t *>(s.h_pin);
    pin[0] = -1;
    HIPT(hipMemcpyAsync(slot(s, S_KDONE), pin, 8, hipMemcpyHostToDevice, s.stream));
    int stop = 0;
    for (int i = 0; i < 2; ++i) TRY(do_iteration(c, 0.0, &stop, /*gated=*/true));
    for (auto &e : s.ev_look) HIPT(hipEventRecord(e, s.stream));  // the gated loop's events: first records too
    const size_t es = (size_t)c->es;
    HIPT(hipMemsetAsync(s.r, 0, (c->fold_p ? c->lda : s.nloc) * es, s.stream));
    HIPT(hipMemsetAsync(s.Ap, 0, s.nloc * es, s.stream));
    HIPT(hipMemsetAsync(s.pfull, 0, c->lda * es, s.stream));
    if (s.p_alt) HIPT(hipMemsetAsync(s.p_alt, 0, c->lda * es, s.stream));
    HIPT(hipMemsetAsync(s.scal, 0, kScalSlots * 8, s.stream));
    HIPT(hipStreamSynchronize(s.stream));
    reset_solve_state(c, ST_IDLE);
    // ... and what outlives a solve, or only a later cgx_iterate call sets
    s.x_zero = true;
    c->xd_k0 = c->total_iters = 0;
    c->last_rr = 0.0;
    c->rr_unsummed = false;
    return CGX_OK;
}

}  // namespace cgxh

extern "C" {

int cgx_solve_begin(cgx_ctx *c) {
    const Range range_("cgx_solve_begin");
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    TRY(csr_need_matrix(c, "cgx_solve_begin"));
    if (c->nr) return nrhs_begin(c);
    return do_begin(c);
}

// Convergence-tested iterations without a host round trip per iteration:
// the update kernel decides sqrt(r.r) < eps on the device and records k+1;
// queued later iterations skip themselves.  The host keeps `look` iterations
// in flight and reads the record of an older iteration (pinned memory,
// event-ordered), so at most `look` no-op iterations are ever enqueued.
static int iterate_gated(cgx_ctx *c, int64_t count, double eps, int64_t *done, int *converged) {
    Shard &s0 = c->sh[0];
    // One GPU: one iteration ahead keeps the device fed (its iteration takes
    // longer than the host's enqueue) and enqueues one no-op iteration fewer
    // after the stop; several row blocks: two (the host's enqueue is the
    // longer one at 8 blocks).  profiles/r06_lookahead_ab.jsonl
    const char *la = std::getenv("CGX_LOOKAHEAD");
    const int look_def = c->mode == M_SINGLE ? 1 : 2;
    const int look = std::max(1, std::min(kLookRing - 1, (la && *la) ? std::atoi(la) : look_def));
    const int64_t k0 = c->k;
    int64_t issued = 0, kd = 0;
    volatile int64_t *rec = s0.h_rec;  // {kdone, r.r bits}, stored by the deciding kernel
    // One process (single GPU or row blocks on several): the record may also
    // be read as soon as it appears, without an event, so a GPU that runs
    // ahead of the host's launches (small N) stops the enqueueing after the
    // deciding iteration.  Never in rank mode, where every rank must enqueue
    // the same iterations (their collectives pair up).
    const bool early = c->mode != M_RCCL;
    for (; issued < count && kd == 0; ++issued) {
        if (early && rec[0] != 0) break;
        int stop = 0;
        TRY(do_iteration(c, eps, &stop, /*gated=*/true));
        TRY(set_dev(s0));
        const int64_t ev = issued;  // an event after every iteration
        HIPT(hipEventRecord(s0.ev_look[ev % kLookRing], s0.stream));
        if (ev >= look) {
            TRY(rank_wait_event(c, s0.ev_look[(ev - look) % kLookRing], "an earlier iteration"));
            const int64_t synced = ev - look;  // the last iteration that event covers
            // Only a record left by an iteration the event covers counts: the
            // host-mapped word may already show a later iteration's decision,
            // and acting on that would make the number of enqueued iterations
            // (and so of collectives) depend on timing, rank by rank.  The
            // record's k is the deciding launch's iteration index (dense: the
            // converged iteration + 1, Poisson: the next iteration), so
            // k <= the synced iteration means that launch is covered.
            const int64_t r = rec[0];
            if (r != 0 && r <= k0 + synced) kd = r;
        }
    }
    TRY(sync_all(c));
    const int64_t kdev = rec[0];
    const int64_t did = kdev ? (kdev - k0) : issued;
    c->total_iters += did - issued;  // do_iteration counted every enqueued one
    if (kdev) {
        const int64_t bits = rec[1];
        double rrf;
        std::memcpy(&rrf, &bits, 8);
        c->last_rr = rrf;
        c->k = kdev;
        c->converged = 1;
        c->state = ST_CONVERGED;
        // fused Poisson: the deciding k_poisson_p (iteration kdev) formed
        // r.r_kdev from the slabs' partials into its slot before it decided,
        // and the launches after it skip themselves: nothing is left unsummed
        c->rr_unsummed = false;
    } else {
        double rr = 0.0;
        TRY(settle_rr(c));
        TRY(read_scalar(c, S_RR + ring(c->k), &rr));
        c->last_rr = rr;
        // The fused Poisson iteration decides a stop one iteration later (at
        // the start of the next k_poisson_p); the last issued iteration's
        // r.r is tested here.  (The dense kernels already tested it.)
        if (c->fused && eps >= 0.0 && std::sqrt(rr) < eps) {
            c->converged = 1;
            c->state = ST_CONVERGED;
        }
    }
    TRY(poisson_x_finish(c));
    if (done) *done = did;
    if (converged) *converged = c->converged;
    return CGX_OK;
}

static int iterate_calls(cgx_ctx *c, int64_t count, double eps, int64_t *done, int *converged);

int cgx_iterate(cgx_ctx *c, int64_t count, double eps, int64_t *done, int *converged) {
    const Range range_("cgx_iterate");
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    if (c->state == ST_IDLE) return fail(CGX_ERR_STATE, "cgx_iterate before cgx_solve_begin");
    if (c->iter_failed)
        return fail(CGX_ERR_STATE, "an earlier cgx_iterate failed part-way through iteration %lld: the solve "
                                   "cannot continue (cgx_solve_begin starts a new one)", (long long)c->k);
    TRY(check_x_complete(c));
    const int rc = c->nr ? nrhs_iterate(c, count, eps, done, converged) : iterate_calls(c, count, eps, done, converged);
    if (rc != CGX_OK) {
        // Part of an iteration may have run on some row blocks (or all of
        // r's update without x's): repeating it would apply it twice.  And
        // when x updates were left out (poisson_x_finish not reached), say so
        // at the next use of x instead of handing out an x with terms missing.
        c->iter_failed = true;
        c->x_incomplete = true;
        c->x_deferred = c->fused && c->xd > 1 && (c->k > c->xd_k0 || c->xalpha_pending);
    }
    return rc;
}

static int iterate_calls(cgx_ctx *c, int64_t count, double eps, int64_t *done, int *converged) {
    const char *gv = std::getenv("CGX_GATED");
    const bool gate_ok = !(gv && *gv == '0');
    c->xd_k0 = c->k;
    if (c->state == ST_BEGUN && count > 0 && eps >= 0.0 && !(c->flags & CGX_HOST_STREAM) && gate_ok)
        return iterate_gated(c, count, eps, done, converged);
    int64_t did = 0;
    while (did < count && c->state == ST_BEGUN) {
        int stop = 0;
        TRY(do_iteration(c, eps, &stop));
        TRY(progress_mark(c));
        ++did;
        if (stop) break;
    }
    TRY(settle_rr(c));
    TRY(poisson_x_finish(c));
    if (done) *done = did;
    if (converged) *converged = c->converged;
    return CGX_OK;
}

int cgx_solve(cgx_ctx *c, void *x_inout, double eps, int64_t max_iter, cgx_stats *st) {
    const Range range_("cgx_solve");
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    TRY(csr_need_matrix(c, "cgx_solve"));
    if (c->nr) return nrhs_solve(c, x_inout, eps, max_iter, st);
    if (x_inout) TRY(cgx_set_x(c, x_inout));
    TRY(sync_all(c));
    const auto t0 = std::chrono::steady_clock::now();
    TRY(do_begin(c));
    const int64_t cap = max_iter < 0 ? c->n : max_iter;  // for(k=0; k<ROWS; ++k)
    int64_t done = 0;
    int conv = 0;
    TRY(cgx_iterate(c, cap, eps, &done, &conv));
    TRY(sync_all(c));
    const auto t1 = std::chrono::steady_clock::now();
    c->solve_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (eps < 0.0 && c->k > 0) {
        double rr = 0.0;
        TRY(read_scalar(c, S_RR + ring(c->k), &rr));
        c->last_rr = rr;
    }
    if (x_inout) TRY(cgx_get_x(c, x_inout));
    if (st) TRY(cgx_get_stats(c, st));
    return CGX_OK;
}

int cgx_get_stats(cgx_ctx *c, cgx_stats *st) {
    if (!c || !st) return fail(CGX_ERR_ARG, "NULL argument");
    if (c->nr) return nrhs_get_stats(c, st);
    TRY(sync_all(c));
    TRY(timing_resolve(c));
    st->iterations = c->k;
    st->converged = c->converged;
    // fixed-count iterations read nothing back: the current r.r from its slot
    // (iterate_calls settled a folded Poisson r.r already)
    if (c->state == ST_BEGUN && c->k > 0 && !c->rr_unsummed) TRY(read_scalar(c, S_RR + ring(c->k), &c->last_rr));
    st->rr = c->last_rr;
    st->solve_ms = c->solve_ms;
    st->matvec_ms = c->matvec_ms;
    st->matvec_count = c->matvec_count;
    st->total_iterations = c->total_iters;
    return CGX_OK;
}

int cgx_reset_timing(cgx_ctx *c) {
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    TRY(sync_all(c));
    c->sh[0].ev_used = 0;
    if (c->sh[0].ts_used > 0) {  // drop the stamps recorded so far (warmup)
        TRY(set_dev(c->sh[0]));
        HIPT(hipMemsetAsync(c->sh[0].ts_dev, 0, (size_t)c->sh[0].ts_used * kTsKern * kTsSlot * 8, c->sh[0].stream));
        c->sh[0].ts_used = 0;
    }
    c->ts_prev_start = c->ts_prev_end = 0;
    for (auto &v : c->ph_samples) v.clear();
    c->matvec_ms = 0.0;
    c->matvec_count = 0;
    return CGX_OK;
}

int cgx_get_phase_times(cgx_ctx *c, cgx_phase_times *out) {
    if (!c || !out) return fail(CGX_ERR_ARG, "NULL argument");
    if (!(c->flags & CGX_PHASES)) return fail(CGX_ERR_STATE, "the context was created without CGX_PHASES");
    TRY(sync_all(c));
    TRY(phase_resolve(c));
    for (int q = 0; q < CGX_PH_COUNT; ++q) {
        std::vector<float> v = c->ph_samples[q];
        out->samples[q] = (int64_t)v.size();
        out->median_us[q] = out->mean_us[q] = 0.0;
        if (v.empty()) continue;
        double sum = 0.0;
        for (float t : v) sum += t;
        out->mean_us[q] = sum / (double)v.size();
        std::sort(v.begin(), v.end());
        const size_t h = v.size() / 2;
        out->median_us[q] = (v.size() & 1) ? v[h] : 0.5 * ((double)v[h - 1] + (double)v[h]);
    }
    return CGX_OK;
}

int cgx_synchronize(cgx_ctx *c) {
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    return sync_all(c);
}

void *cgx_stream(cgx_ctx *c) { return c ? (void *)c->sh[0].stream : nullptr; }

int cgx_set_matvec_plan(cgx_ctx *c, int rows_per_wave, int chunks_in_flight, int nontemporal, int blocks_per_cu) {
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    if (c->nr) return nrhs_set_plan(c, rows_per_wave, chunks_in_flight, nontemporal, blocks_per_cu);
    if (c->op == OP_CSR) return csr_set_plan(c, rows_per_wave, chunks_in_flight, nontemporal, blocks_per_cu);
    if (f32ref(c) || c->op != OP_DENSE || (c->flags & CGX_SYMMETRIC))
        return fail(CGX_ERR_ARG, "only the fp64 row-major dense matVec has a tunable plan");
    const int R = rows_per_wave, U = chunks_in_flight;
    if (a32(c)) {
        if (!matvec_a32_plan_ok(R, U, nontemporal))
            return fail(CGX_ERR_ARG, "CGX_A_F32: (rows_per_wave, chunks_in_flight) must be one of (1,4) (1,8) (2,4) "
                                     "(4,2) (4,4) (8,2) and the load policy 2 or 8 (got %d, %d, %d)", R, U,
                        nontemporal);
        for (auto &s : c->sh) {
            TRY(set_dev(s));
            s.plan = plan_matvec_a32(s.dev, s.nloc, R, U, nontemporal, blocks_per_cu, c->lda);
        }
        return CGX_OK;
    }
    if (R != 1 && R != 2 && R != 4 && R != 8) return fail(CGX_ERR_ARG, "rows_per_wave must be 1, 2, 4 or 8");
    if (U != 2 && U != 4 && U != 8) return fail(CGX_ERR_ARG, "chunks_in_flight must be 2, 4 or 8");
    if (nontemporal != 0 && nontemporal != 1 && nontemporal != 2 && nontemporal != 8)
        return fail(CGX_ERR_ARG, "load policy must be 0 (plain), 1 (non-temporal), 2 (pipelined) or 8 (pipelined "
                                 "non-temporal)");
    // The folded iteration keeps p_k in pfull / p_alt by the parity of k, and
    // the other forms keep it in pfull: switching forms inside a solve would
    // multiply a stale p.  A plan that turns the fold off waits for the next
    // cgx_solve_begin.
    if (R > 2 && c->fold_p && c->state == ST_BEGUN)
        return fail(CGX_ERR_STATE, "rows_per_wave %d turns the folded iteration off: not inside a solve "
                                   "(set the plan before cgx_solve_begin)", R);
    for (auto &s : c->sh) {
        TRY(set_dev(s));
        MatvecPlan pl = plan_matvec_f64(s.dev, s.nloc, R, U, nontemporal, blocks_per_cu, c->lda);
        s.plan = pl;
        s.fold_plan = pl;  // the folded matVec follows the same rows per wave and grid (same p.Ap order)
    }
    if (R > 2) c->fold_p = false;  // the folded matVec has one or two rows per wave
    return CGX_OK;
}

int cgx_get_matvec_plan(cgx_ctx *c, int *rows_per_wave, int *chunks_in_flight, int *nontemporal, int *blocks) {
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    const MatvecPlan &pl = c->nr ? c->nr->plan : c->sh[0].plan;
    if (rows_per_wave) *rows_per_wave = pl.R;
    if (chunks_in_flight) *chunks_in_flight = pl.U;
    if (nontemporal) *nontemporal = pl.nt;
    if (blocks) *blocks = pl.blocks;
    return CGX_OK;
}

int cgx_residual_norm(cgx_ctx *c, double *rnorm, double *bnorm) {
    const Range range_("cgx_residual_norm");
    if (!c) return fail(CGX_ERR_ARG, "ctx is NULL");
    if (c->nr)
        return fail(CGX_ERR_ARG, "cgx_residual_norm: an nrhs context has one residual per system (cgx_residual_norms)");
    TRY(csr_need_matrix(c, "cgx_residual_norm"));
    TRY(check_x_complete(c));
    // ||b - A x|| with the current x: allgather x, matVec, residual, two dots.
    TRY(settle_halo(c));
    TRY(exchange_allgather(c, /*from_x=*/true));
    const int tro = out_slot(c, S_LTR, S_TR), tbo = out_slot(c, S_LTB, S_TB);
    for (auto &s : c->sh) {
        TRY(set_dev(s));
        TRY(launch_matvec(c, s, s.pfull, false, 0));
        if (f32ref(c)) {
            HIPT(residual_ref_f32(s.nloc, f32(s.b), f32(s.Ap), f32(s.r), nullptr, s.stream));
            HIPT(dot_ref_f32(s.nloc, f32(s.r), f32(s.r), slot_f32(s, tro), s.stream));
            HIPT(dot_ref_f32(s.nloc, f32(s.b), f32(s.b), slot_f32(s, tbo), s.stream));
        } else {
            HIPT(residual_f64(s.nloc, f64(s.b), f64(s.Ap), f64(s.r), nullptr, slot_f64(s, tro), s.ws, s.stream));
            HIPT(dot_f64(s.nloc, f64(s.b), f64(s.b), slot_f64(s, tbo), s.ws, s.stream));
        }
    }
    TRY(exchange_scalar(c, S_LTR, S_TR));
    TRY(exchange_scalar(c, S_LTB, S_TB));
    double rr = 0.0, bb = 0.0;
    TRY(read_scalar(c, S_TR, &rr));
    TRY(read_scalar(c, S_TB, &bb));
    if (rnorm) *rnorm = std::sqrt(rr);
    if (bnorm) *bnorm = std::sqrt(bb);
    c->state = ST_IDLE;  // r and p were overwritten
    return CGX_OK;
}

}  // extern "C"
