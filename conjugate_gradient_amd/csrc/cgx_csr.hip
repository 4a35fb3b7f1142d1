// cgx_csr.hip -- cgx_create_csr contexts (cgx_ctx.h, OP_CSR): a general sparse
// A in CSR storage on one GPU, fp64.  The context is a cgx_create context
// without the dense A: its vectors, scalars, stream, events and iteration are
// the same, and launch_matvec multiplies with k_csr_mult_f64 (cgx_csr_core.h).
//
// The kernel reads v[col_idx[e]] unchecked, so the structure is checked on the
// host (cgx_csr_check) before anything is uploaded: no path of a context
// reaches the kernel with indices that did not pass.
//
// cgx_set_csr_f32 uploads float values, which stay float on the device in the
// same value buffer (cgx_ctx::csr_f32); every launch that reads the values
// takes them as csr_values(c), and the kernels widen them exactly, so the
// context gives the bits a double-valued one gives on (double)values[e].
//
// cgx_set_precond / cgx_set_precond_diag put n positive values minv on the
// device (1 / diag(A) extracted there, or the caller's); while they are set,
// do_begin and the two update launches run the PCG kernels (cgx_pcg.hip).
// cgx_set_precond_block / cgx_set_precond_block_values put the inverses W of
// A's bs x bs diagonal blocks there instead (extracted on the device, inverted
// on the host by cgx_pcblock.hip, or the caller's), and one more n-vector z;
// the iteration then runs cgx_pcg_block.hip's kernels.
//
// cgx_set_bsr makes a plain cgx_create_csr context block-valued: brow_ptr and
// bcol_idx take the places of row_ptr and col_idx, the values go up in the
// host layout (what the preconditioners' extraction kernels read) and once more,
// re-laid by k_bsr_tile_f64, into the library's own tiled buffer, which is what
// k_bsr_mult_f64 multiplies (cgx_bsmv.hip).  Only launch_matvec, the plan and
// the two extractions know the difference; the next cgx_set_csr /
// cgx_set_csr_f32 makes the context a scalar one again.
//
// cgx_create_csr_multi (cgx_setup.hip) puts the matrix on several row blocks of
// one process: cgx_set_csr splits the host arrays by rows (csr_upload_blocks)
// and builds, per block, the lists of the entries of p it needs from every
// other block (halo_block; cgx_csr_halo_counts / cgx_csr_halo_list run the same
// builder without a GPU).  The iteration is cgx_create_multi's with the SpMV
// per block and gather_indexed (cgx_vector.hip) as the exchange of p.
#include "cgx_ctx.h"

namespace cgxh {

int csr_need_matrix(const cgx_ctx *c, const char *what) {
    if (c->op == OP_CSR && c->csr_nnz < 0)
        return fail(CGX_ERR_STATE, "%s: no matrix yet (cgx_set_csr comes first on a cgx_create_csr context)", what);
    return CGX_OK;
}

int csr_plan_args(int K, int R, int U, int nt) {
    const bool r_ok = R == 1 || R == 2 || R == 4 || R == 8 || R == 16 || R == 32;
    if (!r_ok || U != 1 || !(K == 1 ? spmv_csr_plan_ok(64 / R, nt) : spmm_csr_plan_ok(K, 64 / R, nt)))
        return fail(CGX_ERR_ARG, "%s context: rows_per_wave (64 / T) must be 1, 2, 4, 8, 16 or 32, "
                                 "chunks_in_flight 1 and the load policy 2 or 8 (got %d, %d, %d)",
                    K == 1 ? "cgx_create_csr" : "cgx_create_csr_nrhs", R, U, nt);
    return CGX_OK;
}

int csr_set_plan(cgx_ctx *c, int R, int U, int nt, int blocks_per_cu) {
    if (is_dia(c)) {  // the diagonal kernels' ranges: 64 or 128 rows per wave, U (stored) diagonals in flight
        const DiaKind &dk = dia_kind(c);
        if ((R != 64 && R != 128) || !dk.plan_ok(R / 64, U, nt))
            return fail(CGX_ERR_ARG, "%sdiagonal-valued cgx_create_csr context: rows_per_wave must be 64 or 128, "
                                     "chunks_in_flight 1, 2, 4 or 8 and the load policy 2 or 8 (got %d, %d, %d)",
                        dk.prefix, R, U, nt);
        Shard &s = c->sh[0];
        TRY(set_dev(s));
        s.plan = dk.plan(s.dev, s.nloc, c->dia_ndiag, R / 64, U, nt, blocks_per_cu);
        c->csr_plan_user = true;
        return CGX_OK;
    }
    TRY(csr_plan_args(1, R, U, nt));
    for (auto &s : c->sh) {  // one T for every row block, each block's grid from its own rows
        TRY(set_dev(s));
        if (c->storage == SK_BSR)  // block-valued: T lanes per block row
            s.plan = plan_spmv_bsr(s.dev, s.nloc / c->bsr_bs, c->bsr_nnzb, c->bsr_bs, 64 / R, nt, blocks_per_cu);
        else
            s.plan = plan_spmv_csr(s.dev, s.nloc, c->csr_nnz >= 0 ? c->csr_nnz : c->csr_cap, 64 / R, nt,
                                   blocks_per_cu, c->csr_f32);
    }
    c->csr_plan_user = true;
    return CGX_OK;
}

// ---- the exchange plan of a sparse A over equal row blocks -------------------------
// Block d (rows [d nloc, (d + 1) nloc)) needs, of block q's slice of p, the
// entries its col_idx names: one pass over the block's col_idx marks them, one
// scan of the marks between the lowest and the highest column named writes
// them out in ascending order, source after source (nothing is sorted).
// off[q] .. off[q + 1] is source q's list in `lists` (offsets into q's
// slice); the own block's list is empty.  `mark` is n zero
// bytes on entry and on return.  lists == nullptr: the counts only.
static void halo_block(int64_t n, int S, const int64_t *row_ptr, const int32_t *col_idx, int d,
                       std::vector<uint8_t> &mark, int64_t *off, std::vector<int32_t> *lists) {
    const int64_t nloc = n / S, lo = (int64_t)d * nloc, hi = lo + nloc;
    int64_t cmin = n, cmax = -1;  // the columns the block names: the scan stays inside them
    for (int64_t e = row_ptr[lo]; e < row_ptr[hi]; ++e) {
        const int64_t c = col_idx[e];
        mark[c] = 1;
        cmin = std::min(cmin, c);
        cmax = std::max(cmax, c);
    }
    off[0] = 0;
    if (lists) lists->clear();
    for (int q = 0; q < S; ++q) {
        int64_t cnt = 0;
        uint8_t *m = mark.data() + (int64_t)q * nloc;
        const int64_t j0 = std::max<int64_t>(0, cmin - (int64_t)q * nloc);
        const int64_t j1 = std::min<int64_t>(nloc, cmax + 1 - (int64_t)q * nloc);
        for (int64_t j = j0; j < j1; ++j) {
            if (!m[j]) continue;
            m[j] = 0;
            if (q == d) continue;
            ++cnt;
            if (lists) lists->push_back((int32_t)j);
        }
        off[q + 1] = off[q] + cnt;
    }
}

// What the host-only plan calls check before they read the structure.
static int halo_args(int64_t n, int S, const int64_t *row_ptr, const int32_t *col_idx, const char *what) {
    if (n < 1) return fail(CGX_ERR_ARG, "%s: n must be >= 1 (got %lld)", what, (long long)n);
    if (S < 1 || S > kMaxShards) return fail(CGX_ERR_ARG, "%s: nshards must be in [1, %d] (got %d)", what, kMaxShards, S);
    if (!row_ptr) return fail(CGX_ERR_ARG, "%s: row_ptr is NULL", what);
    if (n % S != 0)
        return fail(CGX_ERR_SHAPE, "%s: %lld rows are not divisible by %d row blocks", what, (long long)n, S);
    const int64_t nnz = row_ptr[n];
    if (nnz < 0) return fail(CGX_ERR_SHAPE, "%s: row_ptr[n] = %lld is negative", what, (long long)nnz);
    return cgx_csr_check(n, nnz, row_ptr, col_idx);
}

// The block kind's W goes (z stays with the context: free_shard); the stream is idle.
static int pc_block_free(cgx_ctx *c) {
    Shard &s = c->sh[0];
    c->pc_bs = 0;
    if (s.pc_w) {
        TRY(set_dev(s));
        HIPT(hipFree(s.pc_w));
        s.pc_w = nullptr;
        s.pc_wld = 0;
    }
    return CGX_OK;
}

// The preconditioner's buffer goes (cgx_set_csr, cgx_set_precond(CGX_PC_NONE)); the stream is idle.
static int pc_drop(cgx_ctx *c) {
    Shard &s = c->sh[0];
    c->pc_kind = CGX_PC_NONE;
    TRY(pc_block_free(c));
    if (s.pc_minv) {
        TRY(set_dev(s));
        HIPT(hipFree(s.pc_minv));
        s.pc_minv = nullptr;
    }
    return CGX_OK;
}

// The context's storage becomes `to`.  A caller's plan (cgx_set_matvec_plan) goes with the move where its
// vocabulary does: CSR and BSR plans both count T lanes per (block) row, a diagonal plan counts rows per lane and
// names its own kind's kernel.
static void csr_storage_to(cgx_ctx *c, Storage to) {
    if (to != c->storage && (is_dia(c) || to == SK_DIA || to == SK_DIA_SYM)) c->csr_plan_user = false;
    c->storage = to;
}

// An upload failed with part of the new matrix on the device: a scalar context with no matrix until the next
// successful upload.
static void csr_no_matrix(cgx_ctx *c) {
    csr_storage_to(c, SK_CSR);
    c->csr_nnz = -1;
    c->state = ST_IDLE;
}

// The end of every successful upload on one block (csr_upload, bsr_upload, dia_upload; the kind's own parameters
// are set): the matrix is of storage `to` with nnz entries, the preconditioner of the old matrix goes, and the plan
// is the caller's T and policy (rows per lane, diagonals in flight and policy) on the new matrix where it carries
// over, the default rule's otherwise.
static int csr_set_storage(cgx_ctx *c, Storage to, int64_t nnz, bool f32) {
    Shard &s = c->sh[0];
    const Storage was = c->storage;
    csr_storage_to(c, to);
    c->csr_nnz = nnz;
    c->csr_f32 = f32;
    TRY(pc_drop(c));  // the diagonal belonged to the old matrix
    const bool user = c->csr_plan_user;
    switch (to) {
        case SK_CSR:
            if (!user && c->nr) c->nr->plan = plan_spmm_csr(s.dev, s.nloc, nnz, nrhs_width(c->nr->nrhs), 0, -1, 0, f32);
            else if (!user) s.plan = plan_spmv_csr(s.dev, s.nloc, nnz, 0, -1, 0, f32);
            else if (was == SK_BSR) s.plan = plan_spmv_csr(s.dev, s.nloc, nnz, 64 / s.plan.R, s.plan.nt, 0, f32);
            break;  // the tiled buffer of a block-valued context stays
        case SK_BSR:
            s.plan = user ? plan_spmv_bsr(s.dev, s.nloc / c->bsr_bs, c->bsr_nnzb, c->bsr_bs, 64 / s.plan.R, s.plan.nt)
                          : plan_spmv_bsr(s.dev, s.nloc / c->bsr_bs, c->bsr_nnzb, c->bsr_bs);
            break;
        case SK_DIA:
        case SK_DIA_SYM:
            s.plan = user ? dia_kind(c).plan(s.dev, s.nloc, c->dia_ndiag, s.plan.R / 64, s.plan.U, s.plan.nt, 0)
                          : dia_kind(c).plan(s.dev, s.nloc, c->dia_ndiag, 0, 0, -1, 0);
            break;
    }
    c->state = ST_IDLE;
    return CGX_OK;
}

// What every call that sets a preconditioner checks first: the context's kind ...
static int pc_need_ctx(const cgx_ctx *c, const char *what) {
    if (!c) return fail(CGX_ERR_ARG, "%s: ctx is NULL", what);
    if (c->op != OP_CSR) return fail(CGX_ERR_ARG, "%s: not a cgx_create_csr context", what);
    // OP_CSR alone does not do: the K-column update kernels have no PCG form
    if (c->nr) return fail(CGX_ERR_ARG, "%s: not with several right-hand sides (a cgx_create_csr_nrhs context)", what);
    // the PCG kernels read their scalars from one block's slots
    if (c->csr_multi) return fail(CGX_ERR_ARG, "%s: not over row blocks (a cgx_create_csr_multi context)", what);
    return CGX_OK;
}
// ... and that it has a matrix.
static int pc_need_csr(const cgx_ctx *c, const char *what) {
    TRY(pc_need_ctx(c, what));
    return csr_need_matrix(c, what);
}

// room for n doubles
static int pc_alloc(const Shard &s, int64_t n, char **out) {
    const hipError_t e = hipMalloc(out, (size_t)n * 8);
    if (e != hipSuccess)
        return fail(CGX_ERR_NOMEM, "hipMalloc(%zu bytes) on device %d: %s", (size_t)n * 8, s.dev, hipGetErrorString(e));
    return CGX_OK;
}

// CGX_PC_JACOBI: 1 / diag(A) from the CSR arrays into a fresh buffer, which
// replaces the context's only when every row passed (k_csr_diag_minv).
static int pc_jacobi(cgx_ctx *c) {
    Shard &s = c->sh[0];
    TRY(sync_all(c));
    TRY(set_dev(s));
    HIPT(preload_kernels(PL_PCG));
    char *fresh = nullptr;
    TRY(pc_alloc(s, c->n, &fresh));
    auto run = [&]() -> int {
        unsigned long long *pin = reinterpret_cast<unsigned long long *>(s.h_pin);
        pin[0] = ~0ull;
        HIPT(hipMemcpyAsync(slot(s, S_PCBAD), pin, 8, hipMemcpyHostToDevice, s.stream));
        unsigned long long *bad_row = static_cast<unsigned long long *>(slot(s, S_PCBAD));
        switch (c->storage) {
            case SK_DIA:
            case SK_DIA_SYM:  // only offset 0 counts: one extraction for both kinds
                HIPT(dia_diag_minv_f64(c->n, c->dia_ndiag, reinterpret_cast<const int32_t *>(s.csr_ci),
                                       f64(s.dia_data), c->dia_ld, f64(fresh), bad_row, s.stream));
                break;
            case SK_BSR:
                HIPT(preload_kernels(PL_BSMV));
                HIPT(bsr_diag_minv_f64(c->n, c->bsr_bs, reinterpret_cast<const int64_t *>(s.csr_rp),
                                       reinterpret_cast<const int32_t *>(s.csr_ci), f64(s.csr_val), f64(fresh), bad_row,
                                       s.stream));
                break;
            case SK_CSR:
                HIPT(csr_diag_minv_f64(c->n, reinterpret_cast<const int64_t *>(s.csr_rp),
                                       reinterpret_cast<const int32_t *>(s.csr_ci), csr_values(c), f64(fresh), bad_row,
                                       s.stream));
                break;
        }
        HIPT(hipMemcpyAsync(pin, slot(s, S_PCBAD), 8, hipMemcpyDeviceToHost, s.stream));
        HIPT(hipStreamSynchronize(s.stream));
        const unsigned long long bad = pin[0];
        if (bad == ~0ull) return CGX_OK;
        HIPT(hipMemcpyAsync(s.h_pin, fresh + bad * 8, 8, hipMemcpyDeviceToHost, s.stream));  // the row's d_i
        HIPT(hipStreamSynchronize(s.stream));
        const double d = s.h_pin[0];
        if (d == 0.0 && std::signbit(d))
            return fail(CGX_ERR_SHAPE, "cgx_set_precond: row %llu has no diagonal entry (d = 0)", bad);
        return fail(CGX_ERR_SHAPE, "cgx_set_precond: row %llu has the diagonal d = %.17g, not finite or not > 0", bad,
                    d);
    };
    const int rc = run();
    if (rc != CGX_OK) {
        (void)hipFree(fresh);
        return rc;
    }
    if (s.pc_minv) HIPT(hipFree(s.pc_minv));
    s.pc_minv = fresh;
    c->pc_kind = CGX_PC_JACOBI;
    c->state = ST_IDLE;
    return pc_block_free(c);
}

static int pc_block_args(const cgx_ctx *c, int bs, const char *what) {
    TRY(pc_need_ctx(c, what));
    if (bs == 1)
        return fail(CGX_ERR_ARG, "%s: bs = 1 is point Jacobi: use cgx_set_precond(ctx, CGX_PC_JACOBI)", what);
    if (bs < 2 || bs > CGX_MAX_PC_BLOCK)
        return fail(CGX_ERR_ARG, "%s: bs must be in [2, %d] (got %d)", what, CGX_MAX_PC_BLOCK, bs);
    return CGX_OK;
}

// CGX_PC_BLOCK from inverse blocks in the host layout (checked by the caller;
// the stream is idle): W goes up in the kernels' layout into a fresh buffer,
// which replaces the context's preconditioner only when everything before
// went well.
static int pc_block_install(cgx_ctx *c, int bs, const double *W) {
    Shard &s = c->sh[0];
    const int64_t n = c->n, nblk = (n + bs - 1) / bs, wld = round_up(nblk, 2);
    std::vector<double> dev;
    try {
        dev.assign((size_t)(bs * bs) * (size_t)wld, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(CGX_ERR_NOMEM, "host allocation failed");
    }
    for (int64_t k = 0; k < nblk; ++k) {
        const int t = (int)std::min<int64_t>(bs, n - k * bs);  // the unused slots of a short block stay +0.0
        for (int i = 0; i < t; ++i)
            for (int j = 0; j < t; ++j) dev[(size_t)(i * bs + j) * wld + k] = W[k * bs * bs + i * bs + j];
    }
    TRY(set_dev(s));
    HIPT(preload_kernels(PL_PCG_BLOCK));
    if (!s.pc_z) TRY(pc_alloc(s, n, &s.pc_z));
    char *fresh = nullptr;
    TRY(pc_alloc(s, (int64_t)dev.size(), &fresh));
    hipError_t e = hipMemcpyAsync(fresh, dev.data(), dev.size() * 8, hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        return fail(CGX_ERR_HIP, "the upload of the inverse blocks: %s", hipGetErrorString(e));
    }
    TRY(pc_drop(c));  // the diagonal kinds' values, or the earlier blocks
    s.pc_w = fresh;
    s.pc_wld = wld;
    c->pc_bs = bs;
    c->pc_kind = CGX_PC_BLOCK;
    c->state = ST_IDLE;
    return CGX_OK;
}

// The matrix of a cgx_create_csr_multi context, after csr_upload's checks: block
// i gets its rows' row_ptr rebased to 0, its slices of col_idx (still global
// columns) and of the values, and its exchange lists (halo_block).  Whatever
// can refuse the call -- a block above its room, a host or a device allocation
// -- comes before the first byte moves: a refused call leaves the earlier
// matrix, its value type and its lists.
static int csr_upload_blocks(cgx_ctx *c, const int64_t *row_ptr, const int32_t *col_idx, const void *values, bool f32,
                             const char *what) {
    const int S = (int)c->sh.size();
    const int64_t n = c->n, nloc = n / S, nnz = row_ptr[n];
    for (int i = 0; i < S; ++i) {
        const int64_t cnt = row_ptr[(i + 1) * nloc] - row_ptr[i * nloc];
        if (cnt > c->csr_cap)
            return fail(CGX_ERR_SHAPE, "%s: row block %d (rows %lld .. %lld) has %lld entries, every block has room "
                                       "for %lld", what, i, (long long)(i * nloc), (long long)((i + 1) * nloc - 1),
                        (long long)cnt, (long long)c->csr_cap);
    }
    std::vector<std::vector<int32_t>> lists((size_t)S);
    std::vector<GatherLists> offs((size_t)S, GatherLists{});
    std::vector<int64_t> counts((size_t)S * S, 0), rp;
    try {
        std::vector<uint8_t> mark((size_t)n, 0);
        rp.resize((size_t)nloc + 1);
        for (int d = 0; d < S; ++d) {
            halo_block(n, S, row_ptr, col_idx, d, mark, offs[d].off, &lists[d]);
            for (int q = 0; q < S; ++q) counts[(size_t)d * S + q] = offs[d].off[q + 1] - offs[d].off[q];
        }
    } catch (const std::bad_alloc &) {
        return fail(CGX_ERR_NOMEM, "host allocation failed");
    }
    TRY(sync_all(c));  // iterations still enqueued read the arrays and the lists
    std::vector<char *> fresh((size_t)S, nullptr);  // list buffers that have to grow
    auto drop_fresh = [&] {
        for (int i = 0; i < S; ++i)
            if (fresh[i] && hipSetDevice(c->sh[i].dev) == hipSuccess) (void)hipFree(fresh[i]);
    };
    for (int i = 0; i < S; ++i) {
        const Shard &s = c->sh[i];
        const size_t need = lists[i].size();
        if ((int64_t)need <= s.halo_cap) continue;
        hipError_t e = hipSetDevice(s.dev);
        if (e == hipSuccess) e = hipMalloc(&fresh[i], need * 4);
        if (e != hipSuccess) {
            fresh[i] = nullptr;
            drop_fresh();
            return fail(CGX_ERR_NOMEM, "hipMalloc(%zu bytes) on device %d: %s", need * 4, s.dev, hipGetErrorString(e));
        }
    }
    const size_t vb = f32 ? 4 : 8;
    const int rc = [&]() -> int {
        for (int i = 0; i < S; ++i) {
            Shard &s = c->sh[i];
            TRY(set_dev(s));
            const int64_t e0 = row_ptr[i * nloc], cnt = row_ptr[(i + 1) * nloc] - e0;
            for (int64_t j = 0; j <= nloc; ++j) rp[j] = row_ptr[i * nloc + j] - e0;
            HIPT(hipMemcpyAsync(s.csr_rp, rp.data(), (size_t)(nloc + 1) * 8, hipMemcpyHostToDevice, s.stream));
            if (cnt > 0) {
                HIPT(hipMemcpyAsync(s.csr_ci, col_idx + e0, (size_t)cnt * 4, hipMemcpyHostToDevice, s.stream));
                HIPT(hipMemcpyAsync(s.csr_val, static_cast<const char *>(values) + (size_t)e0 * vb, (size_t)cnt * vb,
                                    hipMemcpyHostToDevice, s.stream));
            }
            if (!lists[i].empty())
                HIPT(hipMemcpyAsync(fresh[i] ? fresh[i] : s.halo_idx, lists[i].data(), lists[i].size() * 4,
                                    hipMemcpyHostToDevice, s.stream));
            HIPT(hipStreamSynchronize(s.stream));  // rp is the next block's staging too
        }
        return CGX_OK;
    }();
    if (rc != CGX_OK) {  // some blocks hold the new rows, some the old: no matrix until the next cgx_set_csr
        drop_fresh();
        csr_no_matrix(c);
        return rc;
    }
    for (int i = 0; i < S; ++i) {
        Shard &s = c->sh[i];
        if (fresh[i]) {
            TRY(set_dev(s));
            if (s.halo_idx) HIPT(hipFree(s.halo_idx));
            s.halo_idx = fresh[i];
            s.halo_cap = (int64_t)lists[i].size();
        }
        s.halo = offs[i];
    }
    c->halo_counts = counts;
    c->csr_nnz = nnz;
    c->csr_f32 = f32;
    if (!c->csr_plan_user) {
        // one T for the context, the one a cgx_create_csr context chooses for this matrix (n, nnz);
        // each block's grid from its own rows
        TRY(set_dev(c->sh[0]));
        const MatvecPlan whole = plan_spmv_csr(c->sh[0].dev, n, nnz, 0, -1, 0, f32);
        for (auto &s : c->sh) {
            TRY(set_dev(s));
            s.plan = plan_spmv_csr(s.dev, s.nloc, nnz, 64 / whole.R, whole.nt, 0, f32);
        }
    }
    c->state = ST_IDLE;
    return CGX_OK;
}

// cgx_set_csr (f32 = false: values is double[nnz]) and cgx_set_csr_f32 (float[nnz]):
// the same checks in the same order, then the upload.  Float values take the
// first 4 nnz bytes of the value buffer and stay float there; the context's
// value type changes only once everything is on the device.
static int csr_upload(cgx_ctx *c, const int64_t *row_ptr, const int32_t *col_idx, const void *values, bool f32,
                      const char *what) {
    if (!c) return fail(CGX_ERR_ARG, "%s: ctx is NULL", what);
    if (c->op != OP_CSR) return fail(CGX_ERR_ARG, "%s: not a cgx_create_csr context", what);
    if (!row_ptr) return fail(CGX_ERR_ARG, "%s: row_ptr is NULL", what);
    const int64_t nnz = row_ptr[c->n];  // the entry count a valid row_ptr states; the check below tests the rest
    if (nnz < 0) return fail(CGX_ERR_SHAPE, "%s: row_ptr[n] = %lld is negative", what, (long long)nnz);
    if (nnz > c->csr_cap && !c->csr_multi)  // row blocks: the room is per block, checked once the structure stands
        return fail(CGX_ERR_SHAPE, "%s: %lld entries, the context has room for %lld", what, (long long)nnz,
                    (long long)c->csr_cap);
    if (nnz > 0 && (!col_idx || !values)) return fail(CGX_ERR_ARG, "%s: col_idx / values is NULL", what);
    TRY(cgx_csr_check(c->n, nnz, row_ptr, col_idx));  // nothing is uploaded when it fails
    if (c->csr_multi) return csr_upload_blocks(c, row_ptr, col_idx, values, f32, what);
    Shard &s = c->sh[0];
    TRY(sync_all(c));  // iterations still enqueued read the arrays
    TRY(set_dev(s));
    HIPT(hipMemcpyAsync(s.csr_rp, row_ptr, (size_t)(c->n + 1) * 8, hipMemcpyHostToDevice, s.stream));
    if (nnz > 0) {
        HIPT(hipMemcpyAsync(s.csr_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, s.stream));
        HIPT(hipMemcpyAsync(s.csr_val, values, (size_t)nnz * (f32 ? 4 : 8), hipMemcpyHostToDevice, s.stream));
    }
    HIPT(hipStreamSynchronize(s.stream));
    return csr_set_storage(c, SK_CSR, nnz, f32);
}

// What cgx_csr_check and cgx_bsr_check test, under the caller's names.
struct StructureNames {
    const char *fn, *n, *nnz, *rp, *ci, *row;
};
static int structure_check(const StructureNames &w, int64_t n, int64_t nnz, const int64_t *row_ptr,
                           const int32_t *col_idx) {
    if (n < 1 || nnz < 0) return fail(CGX_ERR_ARG, "%s: %s must be >= 1 and %s >= 0", w.fn, w.n, w.nnz);
    if (!row_ptr || (nnz > 0 && !col_idx)) return fail(CGX_ERR_ARG, "%s: NULL pointer", w.fn);
    if (row_ptr[0] != 0)
        return fail(CGX_ERR_SHAPE, "%s: %s[0] = %lld, must be 0", w.fn, w.rp, (long long)row_ptr[0]);
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i])
            return fail(CGX_ERR_SHAPE, "%s: %s decreases at %s %lld (%lld -> %lld)", w.fn, w.rp, w.row, (long long)i,
                        (long long)row_ptr[i], (long long)row_ptr[i + 1]);
    if (row_ptr[n] != nnz)
        return fail(CGX_ERR_SHAPE, "%s: %s[%s] = %lld, must be %s = %lld", w.fn, w.rp, w.n, (long long)row_ptr[n],
                    w.nnz, (long long)nnz);
    for (int64_t e = 0; e < nnz; ++e)
        if (col_idx[e] < 0 || (int64_t)col_idx[e] >= n)
            return fail(CGX_ERR_SHAPE, "%s: %s[%lld] = %d outside [0, %lld)", w.fn, w.ci, (long long)e,
                        (int)col_idx[e], (long long)n);
    return CGX_OK;
}

// cgx_set_bsr, after its checks: the arrays go up, the values once in the host
// layout and once re-laid for the kernel.  A tiled buffer that has to grow is
// allocated before the first byte moves, so a refusal leaves the earlier matrix.
static int bsr_upload(cgx_ctx *c, int bs, int64_t nnzb, const int64_t *brow_ptr, const int32_t *bcol_idx,
                      const double *values) {
    Shard &s = c->sh[0];
    const int64_t nb = c->n / bs, need = bsr_tiled_count(nnzb, bs);
    TRY(sync_all(c));  // iterations still enqueued read the arrays
    TRY(set_dev(s));
    HIPT(preload_kernels(PL_BSMV));
    char *fresh = nullptr;
    if (need > s.bsr_cap) {
        const hipError_t e = hipMalloc(&fresh, (size_t)need * 8);
        if (e != hipSuccess)
            return fail(CGX_ERR_NOMEM, "hipMalloc(%zu bytes) on device %d: %s", (size_t)need * 8, s.dev,
                        hipGetErrorString(e));
    }
    char *tiled = fresh ? fresh : s.bsr_val;
    const int rc = [&]() -> int {
        HIPT(hipMemcpyAsync(s.csr_rp, brow_ptr, (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, s.stream));
        if (nnzb > 0) {
            HIPT(hipMemcpyAsync(s.csr_ci, bcol_idx, (size_t)nnzb * 4, hipMemcpyHostToDevice, s.stream));
            HIPT(hipMemcpyAsync(s.csr_val, values, (size_t)nnzb * bs * bs * 8, hipMemcpyHostToDevice, s.stream));
            HIPT(bsr_tile_values_f64(nnzb, bs, f64(s.csr_val), f64(tiled), s.stream));
        }
        HIPT(hipStreamSynchronize(s.stream));
        return CGX_OK;
    }();
    if (rc != CGX_OK) {  // part of the new matrix is on the device: no matrix until the next cgx_set_csr / cgx_set_bsr
        if (fresh) (void)hipFree(fresh);
        csr_no_matrix(c);
        return rc;
    }
    if (fresh) {
        if (s.bsr_val) HIPT(hipFree(s.bsr_val));
        s.bsr_val = fresh;
        s.bsr_cap = need;
    }
    c->bsr_bs = bs;
    c->bsr_nnzb = nnzb;
    return csr_set_storage(c, SK_BSR, nnzb * bs * bs, /*f32=*/false);
}

// cgx_set_dia, after its checks: the offsets go into col_idx's place, the
// diagonals at an even pitch (the 16-byte loads of two rows per lane) into the
// context's values where they fit, otherwise into memory of the library's own,
// which is allocated before the first byte moves, so a refusal leaves the
// earlier matrix.  sym: cgx_set_dia_sym, the same arrays read as the upper diagonals.
static int dia_upload(cgx_ctx *c, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld, bool sym) {
    Shard &s = c->sh[0];
    const int64_t pitch = round_up(c->n, 2), need = ndiag * pitch;  // ndiag n <= csr_cap: no overflow
    TRY(sync_all(c));  // iterations still enqueued read the arrays
    TRY(set_dev(s));
    HIPT(preload_kernels(kDiaKinds[sym].preload_ctx));
    char *fresh = nullptr;
    if (need > c->csr_cap && need > s.dia_cap) {
        const hipError_t e = hipMalloc(&fresh, (size_t)need * 8);
        if (e != hipSuccess)
            return fail(CGX_ERR_NOMEM, "hipMalloc(%zu bytes) on device %d: %s", (size_t)need * 8, s.dev,
                        hipGetErrorString(e));
    }
    char *dst = need <= c->csr_cap ? s.csr_val : fresh ? fresh : s.dia_val;
    const int rc = [&]() -> int {
        if (ndiag > 0) {
            HIPT(hipMemcpyAsync(s.csr_ci, offsets, (size_t)ndiag * 4, hipMemcpyHostToDevice, s.stream));
            HIPT(hipMemcpy2DAsync(dst, (size_t)pitch * 8, data, (size_t)ld * 8, (size_t)c->n * 8, (size_t)ndiag,
                                  hipMemcpyHostToDevice, s.stream));
        }
        HIPT(hipStreamSynchronize(s.stream));
        return CGX_OK;
    }();
    if (rc != CGX_OK) {  // part of the new matrix is on the device: no matrix until the next cgx_set_csr / cgx_set_dia
        if (fresh) (void)hipFree(fresh);
        csr_no_matrix(c);
        return rc;
    }
    if (fresh) {
        if (s.dia_val) HIPT(hipFree(s.dia_val));
        s.dia_val = fresh;
        s.dia_cap = need;
    }
    s.dia_data = dst;
    c->dia_ndiag = ndiag;
    c->dia_ld = pitch;
    return csr_set_storage(c, sym ? SK_DIA_SYM : SK_DIA, ndiag * c->n, /*f32=*/false);
}

// cgx_set_dia (sym = false) and cgx_set_dia_sym: the same checks in the same order, then the upload.  The room is
// counted in stored diagonals, not in the expansion's.
static int dia_set(cgx_ctx *c, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld, bool sym,
                   const char *what) {
    if (!c) return fail(CGX_ERR_ARG, "%s: ctx is NULL", what);
    if (c->op != OP_CSR) return fail(CGX_ERR_ARG, "%s: not a cgx_create_csr context", what);
    if (c->nr)
        return fail(CGX_ERR_ARG, "%s: not with several right-hand sides (a cgx_create_csr_nrhs context): batched DIA "
                                 "is not built", what);
    if (c->csr_multi)
        return fail(CGX_ERR_ARG, "%s: not over row blocks (a cgx_create_csr_multi context): DIA over row blocks is "
                                 "not built", what);
    if (ndiag < 0) return fail(CGX_ERR_ARG, "%s: ndiag must be >= 0 (got %lld)", what, (long long)ndiag);
    if (ndiag > 0 && (!offsets || !data)) return fail(CGX_ERR_ARG, "%s: offsets / data is NULL", what);
    if (ld < c->n) return fail(CGX_ERR_SHAPE, "%s: ld = %lld is below n = %lld", what, (long long)ld, (long long)c->n);
    if (ndiag > c->csr_cap / c->n)  // ndiag n > the room, without the product's overflow
        return fail(CGX_ERR_SHAPE, "%s: %lld %s of %lld rows are %.0f entries, the context has room for %lld", what,
                    (long long)ndiag, kDiaKinds[sym].noun, (long long)c->n, (double)ndiag * (double)c->n,
                    (long long)c->csr_cap);
    TRY(kDiaKinds[sym].check(c->n, ndiag, offsets));  // nothing is uploaded when it fails
    return dia_upload(c, ndiag, offsets, data, ld, sym);
}

// cgx_spmv_dia / cgx_spmv_dia_sym
static int spmv_dia_any(int64_t n, int64_t ndiag, const void *offsets, const void *data, int64_t ld, const void *v,
                        void *out, void *stream, bool sym, const char *what) {
    if (n < 0 || ndiag < 0) return fail(CGX_ERR_SHAPE, "%s: bad shape", what);
    if (ld < n) return fail(CGX_ERR_SHAPE, "%s: ld = %lld is below n = %lld", what, (long long)ld, (long long)n);
    if ((ndiag > 0 && (!offsets || !data)) || !v || !out) return fail(CGX_ERR_ARG, "%s: NULL pointer", what);
    const DiaKind &dk = kDiaKinds[sym];
    int dev = 0;
    HIPT(hipGetDevice(&dev));
    RedWs ws;
    TRY(dev_ws(&ws));
    HIPT(preload_kernels(dk.preload_spmv));
    const MatvecPlan pl = dk.plan(dev, n, ndiag, 0, 0, -1, 0);  // the default rule unless the kind's env names a plan
    HIPT(dk.spmv(pl, static_cast<const int32_t *>(offsets), static_cast<const double *>(data), ld, n, ndiag,
                 static_cast<const double *>(v), static_cast<double *>(out), nullptr, nullptr, ws,
                 static_cast<hipStream_t>(stream), nullptr, nullptr));
    return CGX_OK;
}

// cgx_spmv_csr / cgx_spmv_csr_f32
static int spmv_csr_any(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx, CsrValues values,
                        const void *v, void *out, void *stream, const char *what) {
    if (rows < 0 || cols < 0) return fail(CGX_ERR_SHAPE, "%s: bad shape", what);
    if (!row_ptr || !col_idx || !values.p || !v || !out) return fail(CGX_ERR_ARG, "%s: NULL pointer", what);
    int dev = 0;
    HIPT(hipGetDevice(&dev));
    RedWs ws;
    TRY(dev_ws(&ws));
    // the entry count lives on the device: T comes from CGX_SPMV_PLAN or, without it, is 8
    const MatvecPlan pl = plan_spmv_csr(dev, rows, /*nnz=*/-1, 0, -1, 0, values.f32);
    HIPT(spmv_csr_f64(pl, static_cast<const int64_t *>(row_ptr), static_cast<const int32_t *>(col_idx), values, rows,
                      static_cast<const double *>(v), static_cast<double *>(out), nullptr, nullptr, ws,
                      static_cast<hipStream_t>(stream)));
    return CGX_OK;
}

// cgx_spmm_csr / cgx_spmm_csr_f32
static int spmm_csr_any(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx, CsrValues values,
                        int nrhs, const void *V, int64_t ldv, void *Out, int64_t ldo, void *stream, const char *what) {
    if (nrhs < 1 || nrhs > CGX_MAX_NRHS)
        return fail(CGX_ERR_ARG, "%s: nrhs must be in [1, %d] (got %d)", what, CGX_MAX_NRHS, nrhs);
    if (!row_ptr || !col_idx || !values.p || !V || !Out) return fail(CGX_ERR_ARG, "%s: NULL pointer", what);
    if (rows < 0 || cols < 0 || (nrhs > 1 && (ldv < cols || ldo < rows)))
        return fail(CGX_ERR_SHAPE, "%s: bad shape", what);
    int dev = 0;
    HIPT(hipGetDevice(&dev));
    const RedWs none{nullptr, nullptr};  // no fused dot: no reduction scratch
    // the entry count lives on the device: T comes from CGX_SPMM_PLAN or, without it, is 8
    const MatvecPlan pl = plan_spmm_csr(dev, rows, /*nnz=*/-1, nrhs_width(nrhs), 0, -1, 0, values.f32);
    HIPT(spmm_csr_f64(pl, static_cast<const int64_t *>(row_ptr), static_cast<const int32_t *>(col_idx), values, rows,
                      nrhs, static_cast<const double *>(V), ldv, static_cast<double *>(Out), ldo, nullptr, 0, nullptr,
                      none, static_cast<hipStream_t>(stream)));
    return CGX_OK;
}

}  // namespace cgxh

extern "C" {

int cgx_precond_diag_check(int64_t n, const double *minv) {
    if (n < 1) return fail(CGX_ERR_ARG, "cgx_precond_diag_check: n must be >= 1");
    if (!minv) return fail(CGX_ERR_ARG, "cgx_precond_diag_check: NULL pointer");
    for (int64_t i = 0; i < n; ++i)
        if (!(std::isfinite(minv[i]) && minv[i] > 0.0))
            return fail(CGX_ERR_SHAPE, "cgx_precond_diag_check: minv[%lld] = %.17g is not finite or not > 0",
                        (long long)i, minv[i]);
    return CGX_OK;
}

int cgx_set_precond(cgx_ctx *c, int kind) {
    const Range range_("cgx_set_precond");
    TRY(pc_need_csr(c, "cgx_set_precond"));
    if (kind == CGX_PC_DIAG)
        return fail(CGX_ERR_ARG, "cgx_set_precond: CGX_PC_DIAG takes its values through cgx_set_precond_diag");
    if (kind != CGX_PC_NONE && kind != CGX_PC_JACOBI)
        return fail(CGX_ERR_ARG, "cgx_set_precond: kind must be CGX_PC_NONE or CGX_PC_JACOBI (got %d)", kind);
    if (kind == CGX_PC_JACOBI) return pc_jacobi(c);
    TRY(sync_all(c));  // iterations still enqueued read minv
    TRY(pc_drop(c));
    c->state = ST_IDLE;
    return CGX_OK;
}

int cgx_set_precond_diag(cgx_ctx *c, const double *minv) {
    const Range range_("cgx_set_precond_diag");
    TRY(pc_need_csr(c, "cgx_set_precond_diag"));
    if (!minv) return fail(CGX_ERR_ARG, "cgx_set_precond_diag: minv is NULL");
    TRY(cgx_precond_diag_check(c->n, minv));  // nothing changes when it fails
    Shard &s = c->sh[0];
    TRY(sync_all(c));
    TRY(set_dev(s));
    HIPT(preload_kernels(PL_PCG));
    if (!s.pc_minv) TRY(pc_alloc(s, c->n, &s.pc_minv));
    HIPT(hipMemcpyAsync(s.pc_minv, minv, (size_t)c->n * 8, hipMemcpyHostToDevice, s.stream));
    HIPT(hipStreamSynchronize(s.stream));
    c->pc_kind = CGX_PC_DIAG;
    c->state = ST_IDLE;
    return pc_block_free(c);
}

int cgx_set_precond_block(cgx_ctx *c, int bs) {
    const Range range_("cgx_set_precond_block");
    TRY(pc_block_args(c, bs, "cgx_set_precond_block"));
    TRY(csr_need_matrix(c, "cgx_set_precond_block"));
    Shard &s = c->sh[0];
    const int64_t nblk = (c->n + bs - 1) / bs;
    const size_t cnt = (size_t)nblk * bs * bs;
    std::vector<double> D, W;
    try {
        D.resize(cnt);
        W.resize(cnt);
    } catch (const std::bad_alloc &) {
        return fail(CGX_ERR_NOMEM, "host allocation failed");
    }
    TRY(sync_all(c));
    TRY(set_dev(s));
    HIPT(preload_kernels(PL_PCG_BLOCK));
    char *dD = nullptr;
    TRY(pc_alloc(s, (int64_t)cnt, &dD));
    auto extract = [&]() -> int {
        switch (c->storage) {  // the same blocks from every storage
            case SK_DIA:
            case SK_DIA_SYM:  // from the diagonals (cgx_dia.hip), or the upper diagonals and their mirrors (cgx_dia_sym.hip)
                HIPT(dia_kind(c).diag_blocks(c->n, bs, c->dia_ndiag, reinterpret_cast<const int32_t *>(s.csr_ci),
                                             f64(s.dia_data), c->dia_ld, f64(dD), s.stream));
                break;
            case SK_BSR:  // from the BSR arrays, for any bs (cgx_bsmv.hip)
                HIPT(bsr_diag_blocks_f64(c->n, c->bsr_bs, bs, reinterpret_cast<const int64_t *>(s.csr_rp),
                                         reinterpret_cast<const int32_t *>(s.csr_ci), f64(s.csr_val), f64(dD),
                                         s.stream));
                break;
            case SK_CSR:
                HIPT(csr_diag_blocks_f64(c->n, bs, reinterpret_cast<const int64_t *>(s.csr_rp),
                                         reinterpret_cast<const int32_t *>(s.csr_ci), csr_values(c), f64(dD),
                                         s.stream));
                break;
        }
        HIPT(hipMemcpyAsync(D.data(), dD, cnt * 8, hipMemcpyDeviceToHost, s.stream));
        HIPT(hipStreamSynchronize(s.stream));
        return CGX_OK;
    };
    const int rc = extract();
    (void)hipFree(dD);
    TRY(rc);
    // nothing has changed yet: a block that is not positive definite leaves the context as it was
    TRY(cgx_precond_block_invert(c->n, bs, D.data(), W.data()));
    TRY(cgx_precond_block_check(c->n, bs, W.data()));  // an inverse that overflowed
    return pc_block_install(c, bs, W.data());
}

int cgx_set_precond_block_values(cgx_ctx *c, int bs, const double *W) {
    const Range range_("cgx_set_precond_block_values");
    TRY(pc_block_args(c, bs, "cgx_set_precond_block_values"));
    if (!W) return fail(CGX_ERR_ARG, "cgx_set_precond_block_values: W is NULL");
    TRY(csr_need_matrix(c, "cgx_set_precond_block_values"));
    TRY(cgx_precond_block_check(c->n, bs, W));  // nothing changes when it fails
    TRY(sync_all(c));
    return pc_block_install(c, bs, W);
}

int cgx_get_precond_block(cgx_ctx *c, int *bs, double *W) {
    if (!c || !bs) return fail(CGX_ERR_ARG, "cgx_get_precond_block: NULL argument");
    if (c->op != OP_CSR) return fail(CGX_ERR_ARG, "cgx_get_precond_block: not a cgx_create_csr context");
    if (c->pc_kind != CGX_PC_BLOCK)
        return fail(CGX_ERR_STATE, "cgx_get_precond_block: the preconditioner is not CGX_PC_BLOCK");
    const int b = c->pc_bs;
    if (W) {
        Shard &s = c->sh[0];
        const int64_t n = c->n, nblk = (n + b - 1) / b, wld = s.pc_wld;
        std::vector<double> dev;
        try {
            dev.resize((size_t)(b * b) * (size_t)wld);
        } catch (const std::bad_alloc &) {
            return fail(CGX_ERR_NOMEM, "host allocation failed");
        }
        TRY(set_dev(s));
        HIPT(hipMemcpyAsync(dev.data(), s.pc_w, dev.size() * 8, hipMemcpyDeviceToHost, s.stream));
        HIPT(hipStreamSynchronize(s.stream));
        for (int64_t k = 0; k < nblk; ++k)
            for (int i = 0; i < b; ++i)
                for (int j = 0; j < b; ++j) W[k * b * b + i * b + j] = dev[(size_t)(i * b + j) * wld + k];
    }
    *bs = b;
    return CGX_OK;
}

int cgx_get_precond(const cgx_ctx *c, int *kind) {
    if (!c || !kind) return fail(CGX_ERR_ARG, "cgx_get_precond: NULL argument");
    *kind = c->op == OP_CSR ? c->pc_kind : CGX_PC_NONE;
    return CGX_OK;
}

int cgx_get_precond_diag(cgx_ctx *c, double *minv) {
    if (!c || !minv) return fail(CGX_ERR_ARG, "cgx_get_precond_diag: NULL argument");
    if (c->op != OP_CSR) return fail(CGX_ERR_ARG, "cgx_get_precond_diag: not a cgx_create_csr context");
    if (c->pc_kind == CGX_PC_NONE) return fail(CGX_ERR_STATE, "cgx_get_precond_diag: no preconditioner is set");
    if (c->pc_kind == CGX_PC_BLOCK)
        return fail(CGX_ERR_STATE, "cgx_get_precond_diag: the preconditioner is CGX_PC_BLOCK (cgx_get_precond_block)");
    Shard &s = c->sh[0];
    TRY(set_dev(s));
    HIPT(hipMemcpyAsync(minv, s.pc_minv, (size_t)c->n * 8, hipMemcpyDeviceToHost, s.stream));
    HIPT(hipStreamSynchronize(s.stream));
    return CGX_OK;
}

int cgx_csr_check(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col_idx) {
    return structure_check({"cgx_csr_check", "n", "nnz", "row_ptr", "col_idx", "row"}, n, nnz, row_ptr, col_idx);
}

int cgx_bsr_check(int64_t nb, int64_t nnzb, const int64_t *brow_ptr, const int32_t *bcol_idx) {
    return structure_check({"cgx_bsr_check", "nb", "nnzb", "brow_ptr", "bcol_idx", "block row"}, nb, nnzb, brow_ptr,
                           bcol_idx);
}

int cgx_dia_check(int64_t n, int64_t ndiag, const int32_t *offsets) {
    if (n < 1 || ndiag < 0) return fail(CGX_ERR_ARG, "cgx_dia_check: n must be >= 1 and ndiag >= 0");
    if (ndiag > 0 && !offsets) return fail(CGX_ERR_ARG, "cgx_dia_check: NULL pointer");
    for (int64_t k = 0; k < ndiag; ++k)
        if ((int64_t)offsets[k] <= -n || (int64_t)offsets[k] >= n)
            return fail(CGX_ERR_SHAPE, "cgx_dia_check: offsets[%lld] = %d outside (-%lld, %lld)", (long long)k,
                        (int)offsets[k], (long long)n, (long long)n);
    return CGX_OK;
}

int cgx_dia_sym_check(int64_t n, int64_t ndiag, const int32_t *offsets) {
    if (n < 1 || ndiag < 0) return fail(CGX_ERR_ARG, "cgx_dia_sym_check: n must be >= 1 and ndiag >= 0");
    if (ndiag > 0 && !offsets) return fail(CGX_ERR_ARG, "cgx_dia_sym_check: NULL pointer");
    for (int64_t k = 0; k < ndiag; ++k) {
        if (offsets[k] < 0)
            return fail(CGX_ERR_SHAPE, "cgx_dia_sym_check: offsets[%lld] = %d is negative: one-sided storage holds "
                                       "offsets >= 0 (the diagonal -o is the stored diagonal o)", (long long)k,
                        (int)offsets[k]);
        if ((int64_t)offsets[k] >= n)
            return fail(CGX_ERR_SHAPE, "cgx_dia_sym_check: offsets[%lld] = %d outside [0, %lld)", (long long)k,
                        (int)offsets[k], (long long)n);
    }
    return CGX_OK;
}

int cgx_csr_halo_counts(int64_t n, int nshards, const int64_t *row_ptr, const int32_t *col_idx, int64_t *counts) {
    if (!counts) return fail(CGX_ERR_ARG, "cgx_csr_halo_counts: counts is NULL");
    TRY(halo_args(n, nshards, row_ptr, col_idx, "cgx_csr_halo_counts"));
    try {
        std::vector<uint8_t> mark((size_t)n, 0);
        int64_t off[kMaxShards + 1];
        for (int d = 0; d < nshards; ++d) {
            halo_block(n, nshards, row_ptr, col_idx, d, mark, off, nullptr);
            for (int q = 0; q < nshards; ++q) counts[(size_t)d * nshards + q] = off[q + 1] - off[q];
        }
    } catch (const std::bad_alloc &) {
        return fail(CGX_ERR_NOMEM, "host allocation failed");
    }
    return CGX_OK;
}

int cgx_csr_halo_list(int64_t n, int nshards, const int64_t *row_ptr, const int32_t *col_idx, int dst, int src,
                      int32_t *offsets) {
    TRY(halo_args(n, nshards, row_ptr, col_idx, "cgx_csr_halo_list"));
    if (dst < 0 || dst >= nshards || src < 0 || src >= nshards)
        return fail(CGX_ERR_ARG, "cgx_csr_halo_list: blocks (%d, %d) outside [0, %d)", dst, src, nshards);
    try {
        std::vector<uint8_t> mark((size_t)n, 0);
        std::vector<int32_t> lists;
        int64_t off[kMaxShards + 1];
        halo_block(n, nshards, row_ptr, col_idx, dst, mark, off, &lists);
        if (off[src + 1] > off[src]) {
            if (!offsets) return fail(CGX_ERR_ARG, "cgx_csr_halo_list: offsets is NULL");
            std::memcpy(offsets, lists.data() + off[src], (size_t)(off[src + 1] - off[src]) * 4);
        }
    } catch (const std::bad_alloc &) {
        return fail(CGX_ERR_NOMEM, "host allocation failed");
    }
    return CGX_OK;
}

int cgx_get_csr_halo(cgx_ctx *c, int64_t *counts) {
    if (!c || !counts) return fail(CGX_ERR_ARG, "cgx_get_csr_halo: NULL argument");
    if (!c->csr_multi) return fail(CGX_ERR_ARG, "cgx_get_csr_halo: not a cgx_create_csr_multi context");
    TRY(csr_need_matrix(c, "cgx_get_csr_halo"));
    std::memcpy(counts, c->halo_counts.data(), c->halo_counts.size() * 8);
    return CGX_OK;
}

int cgx_gather_indexed(const void *src, const void *idx, int64_t count, void *dst, void *stream) {
    if (count < 0) return fail(CGX_ERR_SHAPE, "cgx_gather_indexed: bad count");
    if (count == 0) return CGX_OK;
    if (!src || !idx || !dst) return fail(CGX_ERR_ARG, "cgx_gather_indexed: NULL pointer");
    PeerTable t{};
    t.p[0] = static_cast<const char *>(src);
    GatherLists one{};
    one.off[1] = count;
    // one source, never the whole-slice form (nloc = -1): every entry goes through its index
    HIPT(gather_indexed(t, 1, -1, -1, one, static_cast<const int32_t *>(idx), -1, static_cast<double *>(dst),
                        static_cast<hipStream_t>(stream)));
    return CGX_OK;
}

int cgx_set_csr(cgx_ctx *c, const int64_t *row_ptr, const int32_t *col_idx, const double *values) {
    const Range range_("cgx_set_csr");
    return csr_upload(c, row_ptr, col_idx, values, /*f32=*/false, "cgx_set_csr");
}

int cgx_set_csr_f32(cgx_ctx *c, const int64_t *row_ptr, const int32_t *col_idx, const float *values) {
    const Range range_("cgx_set_csr_f32");
    return csr_upload(c, row_ptr, col_idx, values, /*f32=*/true, "cgx_set_csr_f32");
}

int cgx_set_bsr(cgx_ctx *c, int bs, const int64_t *brow_ptr, const int32_t *bcol_idx, const double *values) {
    const Range range_("cgx_set_bsr");
    if (!c) return fail(CGX_ERR_ARG, "cgx_set_bsr: ctx is NULL");
    if (!brow_ptr) return fail(CGX_ERR_ARG, "cgx_set_bsr: brow_ptr is NULL");
    if (c->op != OP_CSR) return fail(CGX_ERR_ARG, "cgx_set_bsr: not a cgx_create_csr context");
    if (c->nr)
        return fail(CGX_ERR_ARG, "cgx_set_bsr: not with several right-hand sides (a cgx_create_csr_nrhs context): "
                                 "batched BSR is not built");
    if (c->csr_multi)
        return fail(CGX_ERR_ARG, "cgx_set_bsr: not over row blocks (a cgx_create_csr_multi context): BSR over row "
                                 "blocks is not built");
    if (bs == 1) return fail(CGX_ERR_ARG, "cgx_set_bsr: bs = 1 is scalar CSR: use cgx_set_csr");
    if (bs < 2 || bs > CGX_MAX_BSR_BLOCK)
        return fail(CGX_ERR_ARG, "cgx_set_bsr: bs must be in [2, %d] (got %d)", CGX_MAX_BSR_BLOCK, bs);
    if (c->n % bs != 0)
        return fail(CGX_ERR_SHAPE, "cgx_set_bsr: n = %lld is not divisible by bs = %d", (long long)c->n, bs);
    const int64_t nb = c->n / bs, nnzb = brow_ptr[nb];  // the block count a valid brow_ptr states
    if (nnzb < 0) return fail(CGX_ERR_SHAPE, "cgx_set_bsr: brow_ptr[nb] = %lld is negative", (long long)nnzb);
    if (nnzb > 0 && (!bcol_idx || !values)) return fail(CGX_ERR_ARG, "cgx_set_bsr: bcol_idx / values is NULL");
    if (nnzb > c->csr_cap / (bs * bs))  // nnzb bs^2 > the room, without the product's overflow
        return fail(CGX_ERR_SHAPE, "cgx_set_bsr: %lld blocks of %d x %d are %.0f entries, the context has room for %lld",
                    (long long)nnzb, bs, bs, (double)nnzb * (bs * bs), (long long)c->csr_cap);
    TRY(cgx_bsr_check(nb, nnzb, brow_ptr, bcol_idx));  // nothing is uploaded when it fails
    return bsr_upload(c, bs, nnzb, brow_ptr, bcol_idx, values);
}

int cgx_set_dia(cgx_ctx *c, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld) {
    const Range range_("cgx_set_dia");
    return dia_set(c, ndiag, offsets, data, ld, /*sym=*/false, "cgx_set_dia");
}

int cgx_set_dia_sym(cgx_ctx *c, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld) {
    const Range range_("cgx_set_dia_sym");
    return dia_set(c, ndiag, offsets, data, ld, /*sym=*/true, "cgx_set_dia_sym");
}

int cgx_spmv_dia(int64_t n, int64_t ndiag, const void *offsets, const void *data, int64_t ld, const void *v,
                 void *out, void *stream) {
    return spmv_dia_any(n, ndiag, offsets, data, ld, v, out, stream, /*sym=*/false, "cgx_spmv_dia");
}

int cgx_spmv_dia_sym(int64_t n, int64_t ndiag, const void *offsets, const void *data, int64_t ld, const void *v,
                     void *out, void *stream) {
    return spmv_dia_any(n, ndiag, offsets, data, ld, v, out, stream, /*sym=*/true, "cgx_spmv_dia_sym");
}

int cgx_bsr_tile_values(int64_t nnzb, int bs, const void *values, void *values_tiled, void *stream) {
    if (bs < 2 || bs > CGX_MAX_BSR_BLOCK)
        return fail(CGX_ERR_ARG, "cgx_bsr_tile_values: bs must be in [2, %d] (got %d)", CGX_MAX_BSR_BLOCK, bs);
    if (nnzb < 0) return fail(CGX_ERR_SHAPE, "cgx_bsr_tile_values: bad block count");
    if (!values || !values_tiled) return fail(CGX_ERR_ARG, "cgx_bsr_tile_values: NULL pointer");
    HIPT(bsr_tile_values_f64(nnzb, bs, static_cast<const double *>(values), static_cast<double *>(values_tiled),
                             static_cast<hipStream_t>(stream)));
    return CGX_OK;
}

int cgx_spmv_bsr(int64_t nb, int64_t ncolb, int bs, const void *brow_ptr, const void *bcol_idx,
                 const void *values_tiled, const void *v, void *out, void *stream) {
    if (bs < 2 || bs > CGX_MAX_BSR_BLOCK)
        return fail(CGX_ERR_ARG, "cgx_spmv_bsr: bs must be in [2, %d] (got %d)", CGX_MAX_BSR_BLOCK, bs);
    if (nb < 0 || ncolb < 0) return fail(CGX_ERR_SHAPE, "cgx_spmv_bsr: bad shape");
    if (!brow_ptr || !bcol_idx || !values_tiled || !v || !out) return fail(CGX_ERR_ARG, "cgx_spmv_bsr: NULL pointer");
    if (bs % 2 == 0 && (reinterpret_cast<uintptr_t>(v) & 15))
        return fail(CGX_ERR_ARG, "cgx_spmv_bsr: v must be 16-byte aligned when bs is even (the kernel's loads of v)");
    int dev = 0;
    HIPT(hipGetDevice(&dev));
    RedWs ws;
    TRY(dev_ws(&ws));
    // the block count lives on the device: T comes from CGX_BSMV_PLAN or, without it, is 8
    const MatvecPlan pl = plan_spmv_bsr(dev, nb, /*nnzb=*/-1, bs);
    HIPT(spmv_bsr_f64(pl, bs, static_cast<const int64_t *>(brow_ptr), static_cast<const int32_t *>(bcol_idx),
                      static_cast<const double *>(values_tiled), nb, static_cast<const double *>(v),
                      static_cast<double *>(out), nullptr, nullptr, ws, static_cast<hipStream_t>(stream)));
    return CGX_OK;
}

int cgx_spmv_csr(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx, const void *values,
                 const void *v, void *out, void *stream) {
    return spmv_csr_any(rows, cols, row_ptr, col_idx, CsrValues(values, false), v, out, stream, "cgx_spmv_csr");
}

int cgx_spmv_csr_f32(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx, const float *values,
                     const void *v, void *out, void *stream) {
    return spmv_csr_any(rows, cols, row_ptr, col_idx, CsrValues(values), v, out, stream, "cgx_spmv_csr_f32");
}

int cgx_csr_diag_blocks(int64_t n, int bs, const void *row_ptr, const void *col_idx, const void *values, void *D,
                        void *stream) {
    if (n < 1) return fail(CGX_ERR_SHAPE, "cgx_csr_diag_blocks: bad shape");
    if (bs < 2 || bs > CGX_MAX_PC_BLOCK)
        return fail(CGX_ERR_ARG, "cgx_csr_diag_blocks: bs must be in [2, %d] (got %d)", CGX_MAX_PC_BLOCK, bs);
    if (!row_ptr || !col_idx || !values || !D) return fail(CGX_ERR_ARG, "cgx_csr_diag_blocks: NULL pointer");
    HIPT(csr_diag_blocks_f64(n, bs, static_cast<const int64_t *>(row_ptr), static_cast<const int32_t *>(col_idx),
                             static_cast<const double *>(values), static_cast<double *>(D),
                             static_cast<hipStream_t>(stream)));
    return CGX_OK;
}

int cgx_spmm_csr(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx, const void *values, int nrhs,
                 const void *V, int64_t ldv, void *Out, int64_t ldo, void *stream) {
    return spmm_csr_any(rows, cols, row_ptr, col_idx, CsrValues(values, false), nrhs, V, ldv, Out, ldo, stream,
                        "cgx_spmm_csr");
}

int cgx_spmm_csr_f32(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx, const float *values,
                     int nrhs, const void *V, int64_t ldv, void *Out, int64_t ldo, void *stream) {
    return spmm_csr_any(rows, cols, row_ptr, col_idx, CsrValues(values), nrhs, V, ldv, Out, ldo, stream,
                        "cgx_spmm_csr_f32");
}

}  // extern "C"
