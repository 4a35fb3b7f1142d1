/*
 * cg_hip -- drop-in for the reference's solver programs, host code in C over
 * the libcgx C ABI (include/cgx.h).
 *
 *   serialConjugate.c  : cg_hip matrixA.txt vectorb.txt initialguess.txt
 *   parallel_cg.c      : cg_hip --gpus P matrixA.txt vectorb.txt initialguess.txt
 *   point-to-point_cg.c: cg_hip --gpus P --p2p matrixA.txt vectorb.txt initialguess.txt
 *                        (its exchange: every slice to block 0, then from block 0
 *                        to every block; the scalars summed in rank order)
 *
 * Same positional arguments (serialConjugate.c:48-52, 65-67), same text
 * formats, same stdout lines:
 *   "Computing cg of matrix size : <N*N>"             serialConjugate.c:58
 *   "average clock execution time in seconds: %f"     serialConjugate.c:250
 *   with --gpus > 1 additionally, as parallel_cg.c:123-126 / :334-335:
 *   "collective data distribution time in seconds: %f"  (--p2p: "p2p data
 *    distribution time in seconds: %f", point-to-point_cg.c:133)
 *   "cg method execution time in seconds: %f"
 *   "clock execution time in seconds: %f"
 * Same stopping rule: stop when sqrt(r.r) < EPSILON (1.0e-6,
 * serialConjugate.c:28, :235), at most N iterations (:213).
 *
 * Differences (documented in DESIGN.md s2): N is read at run time (count of
 * values in vectorb, or --dims dimensions.txt, or --n); errors exit non-zero
 * (the reference exits 0, serialConjugate.c:51,56); arithmetic is fp64 unless
 * --fp32-ref, which reproduces serialConjugate.c's float results bit for bit.
 *
 * Extra options: --eps E, --max-iter M, --print-x, --stats, --threads T (text
 * parsing), --spd N [--seed S] (on-device synthetic system instead of files),
 * --symmetric (fp64, one GPU: keep only A's upper-triangle tiles, half the
 * bytes per matVec; CG's A is symmetric by contract, the lower triangle
 * outside the diagonal tiles is not read), --a-fp32 (one GPU: A parsed and
 * kept on the GPU as float, exactly what initialize() reads, with b, x0 and
 * all arithmetic in fp64 -- CGX_A_F32, half the bytes per matVec),
 * --nrhs K (one GPU, fp64: K systems on the one matrix solved together, one
 * read of A per iteration -- cgx_create_nrhs; vectorb and initialguess then
 * hold K*N values, system after system, --print-x prints K*N lines, --stats
 * adds one line per system, and --spd takes b_j from seed S + j),
 * --csr (one GPU, fp64: the dense text matrix is read as always, only its
 * entries that are not +-0 are kept, compressed to CSR row block by row block
 * as they are parsed, and the solve runs through a cgx_create_csr context;
 * --stats adds "nnz: <count>"); with it --jacobi (cgx_set_precond: the
 * solve is preconditioned with 1 / diag(A); --stats adds "precond: jacobi")
 * or --block-jacobi BS (cgx_set_precond_block: preconditioned with the
 * inverses of A's BS x BS diagonal blocks, 2 <= BS <= 8; --stats adds
 * "precond: block-jacobi BS"),
 * --csr-a32 (--csr with the file's values parsed and kept as float, what the
 * reference's fscanf("%f") holds, on the host and on the GPU: cgx_set_csr_f32,
 * 8 bytes per entry streamed in place of 12, all arithmetic still fp64 on the
 * exactly widened values; takes --jacobi or --block-jacobi BS as --csr does and
 * is given without --csr; --stats adds "values: float"),
 * --bsr BS (with --csr, 2 <= BS <= 8 dividing N: every BS x BS block of the
 * matrix that holds an entry is kept whole, zero-filled, and the solve runs
 * through cgx_set_bsr and the block kernel; takes --jacobi or --block-jacobi
 * as --csr does, not --csr-a32; --stats adds "nnzb: <count>"),
 * --dia (with --csr: every diagonal of the matrix that holds an entry is kept
 * whole, offsets ascending, zero-filled, and the solve runs through
 * cgx_set_dia and the gather-free diagonal kernel; takes --jacobi or
 * --block-jacobi as --csr does, not --csr-a32 or --bsr; --stats adds
 * "ndiag: <count>"),
 * --dia-sym (with --csr: the matrix laid out as --dia does, then checked for
 * A[i][j] == A[j][i] slot for slot -- the first (i, j) that differs ends the
 * run -- and only the diagonals of offset >= 0 kept; the solve runs through
 * cgx_set_dia_sym and the one-sided diagonal kernel, each stored value read
 * once for both triangles; options and output as --dia's, "ndiag: <count>" the
 * stored count; not with --csr-a32, --bsr or --dia).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <time.h>
#include <unistd.h>

#include "cgx.h"
#include "cgx_textio.h"

#define EPSILON_DEFAULT 1.0e-6 /* serialConjugate.c:28 */

/* The matrix buffer: anonymous memory 2 MiB-aligned with transparent huge
 * pages requested (CGX_CLI_HUGEPAGES=0: plain malloc).  The parse threads
 * fault it in 512x fewer pages, and releasing it is one short munmap
 * instead of freeing 4-KiB pages one by one (~30 ms for 268 MB). */
typedef struct {
    void *p;     /* aligned start */
    void *base;  /* mapping (or malloc block) */
    size_t len;  /* mapping length; 0 = malloc */
} big_buf;

static int big_alloc(big_buf *bb, size_t bytes) {
    const size_t huge = (size_t)2 << 20;
    const char *e = getenv("CGX_CLI_HUGEPAGES");
    memset(bb, 0, sizeof *bb);
    if (bytes >= huge && !(e && !strcmp(e, "0"))) {
        const size_t len = bytes + huge;
        void *m = mmap(NULL, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m != MAP_FAILED) {
            uintptr_t a = ((uintptr_t)m + huge - 1) & ~(uintptr_t)(huge - 1);
            (void)madvise((void *)a, bytes, MADV_HUGEPAGE);
            bb->p = (void *)a;
            bb->base = m;
            bb->len = len;
            return 0;
        }
    }
    bb->p = bb->base = malloc(bytes ? bytes : 1);
    return bb->p ? 0 : -1;
}

static void big_free(big_buf *bb) {
    if (bb->len) munmap(bb->base, bb->len);
    else free(bb->base);
    memset(bb, 0, sizeof *bb);
}

/* Buffers released on a helper thread, off the critical path: the matrix
 * (or the ring A streamed through) and the mapping of A's text file.  Two
 * munmaps of a GiB or more serialise on the process's mm lock with anything
 * else that maps memory (the b and x0 reads), so this starts after them. */
typedef struct {
    big_buf buf;
    cgx_text *text;
} release_job;

static void *release_buf(void *arg) {
    release_job *r = (release_job *)arg;
    cgx_text_close(r->text);
    big_free(&r->buf);
    return NULL;
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static void usage(const char *prog) {
    fprintf(stderr,
            "usage: %s [--gpus P [--p2p]] [--fp32-ref | --symmetric | --a-fp32] [--eps E] [--max-iter M] [--dims FILE] [--n N]\n"
            "          [--threads T] [--print-x] [--stats] matrixA vectorb initialguess\n"
            "       %s --spd N [--seed S] [--gpus P] [--a-fp32] [--eps E] [--max-iter M] [--stats]\n"
            "       %s --nrhs K ... (one GPU, fp64: K systems on one matrix; vectorb and initialguess hold K*N values)\n"
            "       %s --csr [--jacobi | --block-jacobi BS] ... (one GPU, fp64: the matrix's non-zero entries only, solved\n"
            "          as a sparse CSR system; --jacobi: preconditioned with 1 / diag(A); --block-jacobi BS: with the\n"
            "          inverses of A's BS x BS diagonal blocks, BS in 2..8)\n"
            "       %s --csr-a32 [--jacobi | --block-jacobi BS] ... (--csr with the values parsed and kept as float, fp64\n"
            "          arithmetic; given without --csr)\n"
            "       %s --csr --bsr BS [--jacobi | --block-jacobi BS] ... (--csr held as dense BS x BS blocks, BS in 2..8\n"
            "          dividing N, multiplied by the block kernel; not with --csr-a32)\n"
            "       %s --csr --dia [--jacobi | --block-jacobi BS] ... (--csr held as the diagonals that hold an entry,\n"
            "          multiplied by the diagonal kernel; not with --csr-a32 or --bsr)\n"
            "       %s --csr --dia-sym [--jacobi | --block-jacobi BS] ... (--csr, symmetric, held as the diagonals of its\n"
            "          upper triangle alone, multiplied by the one-sided diagonal kernel; not with --csr-a32, --bsr or --dia)\n",
            prog, prog, prog, prog, prog, prog, prog, prog);
}

static int die_cgx(int rc, const char *what) {
    fprintf(stderr, "%s failed: %s (%s)\n", what, cgx_strerror(rc), cgx_last_error());
    return 1;
}

static int read_file(const char *path, int64_t count, int as_float, void *out, int threads) {
    int rc = cgx_text_read(path, count, as_float, out, threads);
    if (rc == -1) {
        printf("Could not open file\n"); /* serialConjugate.c:103 */
        fprintf(stderr, "%s: cannot open\n", path);
    } else if (rc == -2) {
        fprintf(stderr, "%s: fewer than %lld numbers\n", path, (long long)count);
    } else if (rc != 0) {
        fprintf(stderr, "%s: malformed number\n", path);
    }
    return rc;
}

/* Context creation (HIP runtime start, device buffers) runs on its own thread
 * while the text files are parsed: the two are independent until the H2D. */
typedef struct {
    int64_t n;
    int gpus, flags, rc;
    int nrhs;  /* > 0: cgx_create_nrhs */
    cgx_ctx *ctx;
    double t_rt, t_done;  /* when the HIP runtime was up / creation finished (now_s) */
    int csr;              /* --csr: cgx_create_csr, once the parse has counted the entries */
    int64_t csr_nnz;      /* < 0: not counted yet (the thread only starts the HIP runtime) */
} create_job;

static void *create_ctx(void *arg) {
    create_job *j = (create_job *)arg;
    int ndev0 = 0;
    cgx_device_count(&ndev0); /* starts the HIP runtime */
    j->t_rt = now_s();
    if (j->csr) {
        if (j->csr_nnz >= 0) j->rc = cgx_create_csr(&j->ctx, j->n, j->csr_nnz, 0, j->flags);
    } else if (j->nrhs > 0) {
        j->rc = cgx_create_nrhs(&j->ctx, j->n, j->nrhs, 0, j->flags);
    } else if (j->gpus == 1) {
        j->rc = cgx_create(&j->ctx, j->n, 0, j->flags);
    } else {
        int devs[32];
        int ndev = 0;
        cgx_device_count(&ndev);
        for (int g = 0; g < j->gpus; ++g) devs[g] = ndev > 0 ? g % ndev : 0;
        j->rc = cgx_create_multi(&j->ctx, j->n, j->gpus, devs, j->flags);
    }
    j->t_done = now_s();
    return NULL;
}

/* A streamed to the GPU row block by row block (parallel_cg.c's MPI_Scatter,
 * :112-113, one block at a time): the main thread parses block k+1 from the
 * indexed file while a copy thread sends block k with cgx_set_rows, through
 * a ring of block buffers, so host memory holds at most CGX_CLI_RING_MB
 * (default 1024) of A and, once the context is up, the H2D runs under the
 * parse.  The ring is one buffer: when the copy thread finds several parsed
 * blocks waiting (the HIP runtime came up after them) it sends the run of
 * them that is contiguous in the ring with one cgx_set_rows, since pageable
 * H2D copies run at ~5 GB/s per 32 MB call and ~20 GB/s per 256 MB call.
 * Blocks are CGX_CLI_BLOCK_MB (default 128) of A.
 * (CGX_CLI_STREAM=0: parse all of A, then one cgx_set_system.) */
typedef struct {
    cgx_text *text;
    int64_t n, block_rows, nblocks;
    int nslots, as_float, threads;
    size_t es;
    big_buf ring;         /* nslots slots of block_rows * n values (huge pages) */
    size_t slot_bytes;
    int *filled;          /* slot holds block filled[s] - 1 (0 = free) */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int abort_rc;         /* the copy side failed: the parse stops */
    pthread_t creator;    /* joined by the copy thread */
    int creator_threaded;
    create_job *job;
    int rc;               /* first cgx_set_rows failure */
    double t_last_h2d;
} a_stream;

static void *stream_copy(void *arg) {
    a_stream *st = (a_stream *)arg;
    if (st->creator_threaded) pthread_join(st->creator, NULL);
    int rc = st->job->rc;
    for (int64_t k = 0; k < st->nblocks && rc == CGX_OK;) {
        const int sl = (int)(k % st->nslots);
        pthread_mutex_lock(&st->mu);
        while (st->filled[sl] != k + 1 && !st->abort_rc) pthread_cond_wait(&st->cv, &st->mu);
        int64_t run = 1; /* parsed blocks k, k+1, ... in consecutive slots */
        while (k + run < st->nblocks && sl + run < st->nslots && st->filled[sl + run] == k + run + 1) ++run;
        const int stop = st->abort_rc;
        pthread_mutex_unlock(&st->mu);
        if (stop) break;
        const int64_t row0 = k * st->block_rows, end = (k + run) * st->block_rows < st->n ? (k + run) * st->block_rows : st->n;
        rc = cgx_set_rows(st->job->ctx, row0, end - row0, (char *)st->ring.p + (size_t)sl * st->slot_bytes, st->n,
                          NULL, NULL);
        pthread_mutex_lock(&st->mu);
        for (int64_t q = 0; q < run; ++q) st->filled[sl + q] = 0;
        pthread_cond_broadcast(&st->cv);
        pthread_mutex_unlock(&st->mu);
        k += run;
    }
    st->t_last_h2d = now_s();
    pthread_mutex_lock(&st->mu);
    st->rc = rc;
    if (rc != CGX_OK && !st->abort_rc) st->abort_rc = 1;
    pthread_cond_broadcast(&st->cv);
    pthread_mutex_unlock(&st->mu);
    return NULL;
}

/* The parse side (main thread).  Returns 0, or the text reader's error. */
static int stream_parse(a_stream *st) {
    for (int64_t k = 0; k < st->nblocks; ++k) {
        const int sl = (int)(k % st->nslots);
        pthread_mutex_lock(&st->mu);
        while (st->filled[sl] != 0 && !st->abort_rc) pthread_cond_wait(&st->cv, &st->mu);
        const int stop = st->abort_rc;
        pthread_mutex_unlock(&st->mu);
        if (stop) return 0; /* the copy side reports its own error */
        const int64_t row0 = k * st->block_rows, rows = row0 + st->block_rows <= st->n ? st->block_rows : st->n - row0;
        const int rc = cgx_text_read_range(st->text, row0 * st->n, rows * st->n, st->as_float,
                                           (char *)st->ring.p + (size_t)sl * st->slot_bytes, st->threads);
        pthread_mutex_lock(&st->mu);
        if (rc != 0) st->abort_rc = 1;
        else st->filled[sl] = (int)(k + 1);
        pthread_cond_broadcast(&st->cv);
        pthread_mutex_unlock(&st->mu);
        if (rc != 0) return rc;
    }
    return 0;
}

/* --csr: A's text parsed row block by row block (the streaming reader's
 * blocks) into one block buffer, and each block's entries that are not +-0
 * appended to the CSR arrays, which grow as needed.  Returns 0, or the text
 * reader's error (-2 short, -3 malformed), or -9 when memory runs out. */
typedef struct {
    int64_t *row_ptr;
    int32_t *col_idx;
    void *values; /* double, or float with --csr-a32 (as_float): parsed, kept and uploaded as such */
    int64_t nnz, cap;
} csr_host;

static int csr_parse(cgx_text *text, int64_t n, int64_t block_rows, void *blk, int threads, csr_host *m,
                     int as_float) {
    const size_t ves = as_float ? sizeof(float) : sizeof(double);
    m->row_ptr = malloc((size_t)(n + 1) * sizeof(int64_t));
    m->cap = 8 * n > 1024 ? 8 * n : 1024;
    m->col_idx = malloc((size_t)m->cap * sizeof(int32_t));
    m->values = malloc((size_t)m->cap * ves);
    m->nnz = 0;
    if (!m->row_ptr || !m->col_idx || !m->values) return -9;
    m->row_ptr[0] = 0;
    for (int64_t row0 = 0; row0 < n; row0 += block_rows) {
        const int64_t rows = row0 + block_rows <= n ? block_rows : n - row0;
        const int rc = cgx_text_read_range(text, row0 * n, rows * n, as_float, blk, threads);
        if (rc != 0) return rc;
        for (int64_t i = 0; i < rows; ++i) {
            if (m->nnz + n > m->cap) { /* room for a full row */
                const int64_t cap = 2 * m->cap > m->nnz + n ? 2 * m->cap : m->nnz + n;
                int32_t *ci = realloc(m->col_idx, (size_t)cap * sizeof(int32_t));
                if (ci) m->col_idx = ci;
                void *va = realloc(m->values, (size_t)cap * ves);
                if (va) m->values = va;
                if (!ci || !va) return -9;
                m->cap = cap;
            }
            /* +0 and -0 are dropped; everything else is an entry */
            if (as_float) {
                const float *row = (const float *)blk + (size_t)i * (size_t)n;
                for (int64_t j = 0; j < n; ++j)
                    if (row[j] != 0.0f) {
                        m->col_idx[m->nnz] = (int32_t)j;
                        ((float *)m->values)[m->nnz++] = row[j];
                    }
            } else {
                const double *row = (const double *)blk + (size_t)i * (size_t)n;
                for (int64_t j = 0; j < n; ++j)
                    if (row[j] != 0.0) {
                        m->col_idx[m->nnz] = (int32_t)j;
                        ((double *)m->values)[m->nnz++] = row[j];
                    }
            }
            m->row_ptr[row0 + i + 1] = m->nnz;
        }
    }
    return 0;
}

/* --bsr BS: the CSR arrays of csr_parse as block CSR -- every BS x BS block
 * that holds an entry, block columns ascending, the rest of a block +0.0
 * (n % bs == 0, values double).  Returns 0, or -9 when memory runs out. */
typedef struct {
    int64_t *brow_ptr;
    int32_t *bcol_idx;
    double *values;
    int64_t nnzb;
} bsr_host;

static int bsr_from_csr(const csr_host *m, int64_t n, int bs, bsr_host *out) {
    const int64_t nb = n / bs;
    const double *val = (const double *)m->values;
    out->brow_ptr = malloc((size_t)(nb + 1) * sizeof(int64_t));
    int64_t *slot = malloc((size_t)nb * sizeof(int64_t)); /* a block column's place in the current block row, or -1 */
    if (!out->brow_ptr || !slot) { free(slot); return -9; }
    for (int64_t c = 0; c < nb; ++c) slot[c] = -1;
    /* pass 1 counts the blocks of every block row, pass 2 places them */
    for (int pass = 0; pass < 2; ++pass) {
        int64_t nnzb = 0;
        for (int64_t I = 0; I < nb; ++I) {
            /* the block columns the bs rows name, ascending: mark, then sweep between the lowest and the highest */
            int64_t lo = nb, hi = -1;
            for (int64_t e = m->row_ptr[I * bs]; e < m->row_ptr[(I + 1) * bs]; ++e) {
                const int64_t c = m->col_idx[e] / bs;
                slot[c] = -2;
                if (c < lo) lo = c;
                if (c > hi) hi = c;
            }
            for (int64_t c = lo; c <= hi; ++c)
                if (slot[c] == -2) {
                    if (pass) out->bcol_idx[nnzb] = (int32_t)c;
                    slot[c] = nnzb++;
                }
            if (pass)
                for (int i = 0; i < bs; ++i)
                    for (int64_t e = m->row_ptr[I * bs + i]; e < m->row_ptr[I * bs + i + 1]; ++e) {
                        const int64_t c = m->col_idx[e] / bs;
                        out->values[(slot[c] * bs + i) * bs + (m->col_idx[e] - c * bs)] = val[e];
                    }
            for (int64_t c = lo; c <= hi; ++c) slot[c] = -1;
            if (!pass) out->brow_ptr[I + 1] = nnzb;
        }
        if (!pass) {
            out->brow_ptr[0] = 0;
            out->nnzb = nnzb;
            out->bcol_idx = malloc((size_t)(nnzb > 0 ? nnzb : 1) * sizeof(int32_t));
            out->values = calloc((size_t)(nnzb > 0 ? nnzb : 1) * (size_t)(bs * bs), sizeof(double));
            if (!out->bcol_idx || !out->values) { free(slot); return -9; }
        }
    }
    free(slot);
    return 0;
}

/* --dia: the CSR arrays of csr_parse by diagonals -- every diagonal that holds
 * an entry, offsets ascending, the rest of a diagonal +0.0; data[k * n + j] =
 * A[j - offsets[k]][j] (values double).  Returns 0, or -9 when memory runs out. */
typedef struct {
    int32_t *offsets;
    double *data;
    int64_t ndiag;
} dia_host;

static int dia_from_csr(const csr_host *m, int64_t n, dia_host *out) {
    const double *val = (const double *)m->values;
    int64_t *slot = malloc((size_t)(2 * n - 1) * sizeof(int64_t)); /* offset o's diagonal at slot[o + n - 1], or -1 */
    if (!slot) return -9;
    for (int64_t d = 0; d < 2 * n - 1; ++d) slot[d] = -1;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = m->row_ptr[i]; e < m->row_ptr[i + 1]; ++e) slot[m->col_idx[e] - i + n - 1] = 0;
    int64_t ndiag = 0;
    for (int64_t d = 0; d < 2 * n - 1; ++d)
        if (slot[d] == 0) slot[d] = ndiag++;
    out->ndiag = ndiag;
    out->offsets = malloc((size_t)(ndiag > 0 ? ndiag : 1) * sizeof(int32_t));
    out->data = calloc((size_t)(ndiag > 0 ? ndiag : 1) * (size_t)n, sizeof(double));
    if (!out->offsets || !out->data) { free(slot); return -9; }
    for (int64_t d = 0; d < 2 * n - 1; ++d)
        if (slot[d] >= 0) out->offsets[slot[d]] = (int32_t)(d - (n - 1));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = m->row_ptr[i]; e < m->row_ptr[i + 1]; ++e)
            out->data[slot[m->col_idx[e] - i + n - 1] * n + m->col_idx[e]] = val[e];
    free(slot);
    return 0;
}

/* --dia-sym: the diagonals of dia_from_csr checked for symmetry -- diagonal -o
 * must equal diagonal +o slot for slot, a diagonal the matrix lacks being +0.0
 * -- and cut down in place to the offsets >= 0, still ascending.  Returns 0, or
 * -1 with the first (i, j) in row order where A[i][j] != A[j][i]. */
static int dia_sym_from_dia(dia_host *m, int64_t n, int64_t *bad_i, int64_t *bad_j) {
    int64_t k0 = 0; /* the first diagonal of offset >= 0 */
    while (k0 < m->ndiag && m->offsets[k0] < 0) ++k0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < m->ndiag; ++k) {
            const int64_t o = m->offsets[k], j = i + o;
            if (o == 0 || j < 0 || j >= n) continue;
            int64_t km = -1; /* the diagonal -o, if the matrix has it */
            for (int64_t q = 0; q < m->ndiag; ++q)
                if (m->offsets[q] == -o) km = q;
            const double a = m->data[k * n + j], at = km >= 0 ? m->data[km * n + i] : 0.0; /* A[i][j], A[j][i] */
            if (a != at) {
                *bad_i = i;
                *bad_j = j;
                return -1;
            }
        }
    for (int64_t k = k0; k < m->ndiag; ++k) m->offsets[k - k0] = m->offsets[k];
    if (k0 > 0 && m->ndiag > k0) memmove(m->data, m->data + k0 * n, (size_t)(m->ndiag - k0) * (size_t)n * sizeof(double));
    m->ndiag -= k0;
    return 0;
}

/* Whole-string numeric option values: "--eps abc" or "--gpus 2x" is an
 * error (exit 2), not a silent 0. */
static int opt_ll(const char *name, const char *v, long long *out) {
    char *end = NULL;
    errno = 0;
    const long long x = strtoll(v, &end, 10);
    if (!*v || *end || errno) { fprintf(stderr, "%s: not an integer: '%s'\n", name, v); return 0; }
    *out = x;
    return 1;
}
static int opt_double(const char *name, const char *v, double *out) {
    char *end = NULL;
    errno = 0;
    const double x = strtod(v, &end);
    if (!*v || *end || errno) { fprintf(stderr, "%s: not a number: '%s'\n", name, v); return 0; }
    *out = x;
    return 1;
}

int main(int argc, char **argv) {
    const double t_prog0 = now_s();
    int gpus = 1, fp32ref = 0, symmetric = 0, print_x = 0, stats = 0, p2p = 0, a_fp32 = 0, csr = 0, jacobi = 0;
    int csr_a32 = 0; /* --csr-a32: becomes csr = 1 once the combinations are checked */
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    int threads = (int)(ncpu < 1 ? 1 : (ncpu > 16 ? 16 : ncpu)); /* text parsing threads */
    double eps = EPSILON_DEFAULT;
    long long max_iter = -1, n_opt = -1, spd_n = -1, nrhs = 0, block_bs = 0; /* block_bs > 0: --block-jacobi */
    long long bsr_bs = 0; /* > 0: --bsr */
    int dia = 0;          /* --dia */
    int dia_sym = 0;      /* --dia-sym: becomes dia = 1 once the combinations are checked */
    unsigned long long seed = 42;
    const char *dims_path = NULL;
    const char *pos[3];
    int npos = 0;

    long long v = 0;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        int has_val = (i + 1 < argc);
        if (!strcmp(a, "--gpus") && has_val) {
            if (!opt_ll(a, argv[++i], &v)) return 2;
            gpus = (v < 0 || v > 1000) ? -1 : (int)v;
        } else if (!strcmp(a, "--fp32-ref")) fp32ref = 1;
        else if (!strcmp(a, "--symmetric")) symmetric = 1;
        else if (!strcmp(a, "--a-fp32")) a_fp32 = 1;
        else if (!strcmp(a, "--p2p")) p2p = 1;
        else if (!strcmp(a, "--csr")) csr = 1;
        else if (!strcmp(a, "--csr-a32")) csr_a32 = 1;
        else if (!strcmp(a, "--jacobi")) jacobi = 1;
        else if (!strcmp(a, "--block-jacobi")) {
            if (has_val && !opt_ll(a, argv[++i], &block_bs)) return 2;
            if (!has_val || block_bs < 2 || block_bs > CGX_MAX_PC_BLOCK) {
                fprintf(stderr, "--block-jacobi must be an integer in [2, %d]\n", CGX_MAX_PC_BLOCK);
                return 2;
            }
        } else if (!strcmp(a, "--bsr")) {
            if (has_val && !opt_ll(a, argv[++i], &bsr_bs)) return 2;
            if (!has_val || bsr_bs < 2 || bsr_bs > CGX_MAX_BSR_BLOCK) {
                fprintf(stderr, "--bsr must be an integer in [2, %d]\n", CGX_MAX_BSR_BLOCK);
                return 2;
            }
        } else if (!strcmp(a, "--dia")) dia = 1;
        else if (!strcmp(a, "--dia-sym")) dia_sym = 1;
        else if (!strcmp(a, "--eps") && has_val) {
            if (!opt_double(a, argv[++i], &eps)) return 2;
        } else if (!strcmp(a, "--max-iter") && has_val) {
            if (!opt_ll(a, argv[++i], &max_iter)) return 2;
        } else if (!strcmp(a, "--dims") && has_val) dims_path = argv[++i];
        else if (!strcmp(a, "--n") && has_val) {
            if (!opt_ll(a, argv[++i], &n_opt)) return 2;
        } else if (!strcmp(a, "--threads") && has_val) {
            if (!opt_ll(a, argv[++i], &v)) return 2;
            threads = v < 1 ? 1 : (v > 256 ? 256 : (int)v);
        } else if (!strcmp(a, "--spd") && has_val) {
            if (!opt_ll(a, argv[++i], &spd_n)) return 2;
        } else if (!strcmp(a, "--nrhs") && has_val) {
            if (!opt_ll(a, argv[++i], &nrhs)) return 2;
            if (nrhs < 1 || nrhs > CGX_MAX_NRHS) { fprintf(stderr, "--nrhs must be in [1, %d]\n", CGX_MAX_NRHS); return 2; }
        } else if (!strcmp(a, "--seed") && has_val) {
            if (!opt_ll(a, argv[++i], &v)) return 2;
            seed = (unsigned long long)v;
        } else if (!strcmp(a, "--print-x")) print_x = 1;
        else if (!strcmp(a, "--stats")) stats = 1;
        else if (!strcmp(a, "-h") || !strcmp(a, "--help")) { usage(argv[0]); return 0; }
        else if (a[0] == '-' && a[1] == '-') { usage(argv[0]); return 2; }
        else if (npos < 3) pos[npos++] = a;
        else npos = 4;
    }
    if (spd_n < 0 && npos != 3) {
        printf("serialCongugate.c requires four (4) files \n"); /* serialConjugate.c:50 */
        usage(argv[0]);
        return 1;
    }
    if (gpus < 1) { fprintf(stderr, "--gpus must be >= 1\n"); return 2; }
    if (gpus > 32) { fprintf(stderr, "--gpus must be <= 32\n"); return 2; }
    if (csr_a32 && (csr || fp32ref || a_fp32 || symmetric || gpus != 1 || p2p || nrhs > 0 || spd_n >= 0)) {
        fprintf(stderr, "--csr-a32 is --csr with float-stored values: it is given alone (no --csr, --fp32-ref, --a-fp32, --symmetric, --gpus, --p2p, --nrhs, --spd)\n");
        return 2;
    }
    if (dia_sym && (csr_a32 || bsr_bs > 0 || dia || !csr)) {
        fprintf(stderr, "--dia-sym holds a --csr matrix by its upper diagonals, double values: it is given with --csr (not --csr-a32, --bsr or --dia)\n");
        return 2;
    }
    if (dia_sym) dia = 1; /* laid out by diagonals first */
    if (bsr_bs > 0 && (csr_a32 || !csr)) {
        fprintf(stderr, "--bsr holds a --csr matrix as dense blocks of double values: it is given with --csr (not --csr-a32)\n");
        return 2;
    }
    if (dia && (csr_a32 || bsr_bs > 0 || !csr)) {
        fprintf(stderr, "--dia holds a --csr matrix by its diagonals, double values: it is given with --csr (not --csr-a32 or --bsr)\n");
        return 2;
    }
    if (csr_a32) csr = 1;
    if (p2p && symmetric) {
        fprintf(stderr, "--p2p is an exchange of several row blocks (--symmetric is one GPU)\n");
        return 2;
    }
    if (symmetric && (fp32ref || gpus != 1)) {
        fprintf(stderr, "--symmetric is fp64 on one GPU (no --fp32-ref, --gpus 1)\n");
        return 2;
    }
    if (a_fp32 && (fp32ref || symmetric || gpus != 1)) {
        fprintf(stderr, "--a-fp32 is float A with fp64 arithmetic on one GPU (no --fp32-ref, no --symmetric, --gpus 1)\n");
        return 2;
    }
    if (nrhs > 0 && (fp32ref || a_fp32 || symmetric || gpus != 1 || p2p)) {
        fprintf(stderr, "--nrhs is fp64 on one GPU with A resident (no --fp32-ref, --a-fp32, --symmetric, --gpus, --p2p)\n");
        return 2;
    }
    if (jacobi && (!csr || fp32ref || a_fp32 || symmetric || gpus != 1 || p2p || nrhs > 0 || spd_n >= 0)) {
        fprintf(stderr, "--jacobi preconditions a --csr solve (fp64 on one GPU from a matrix file: no --fp32-ref, --a-fp32, --symmetric, --gpus, --p2p, --nrhs, --spd)\n");
        return 2;
    }
    if (block_bs > 0 && jacobi) {
        fprintf(stderr, "--block-jacobi and --jacobi are two preconditioners: give one\n");
        return 2;
    }
    if (block_bs > 0 && (!csr || fp32ref || a_fp32 || symmetric || gpus != 1 || p2p || nrhs > 0 || spd_n >= 0)) {
        fprintf(stderr, "--block-jacobi preconditions a --csr solve (fp64 on one GPU from a matrix file: no --fp32-ref, --a-fp32, --symmetric, --gpus, --p2p, --nrhs, --spd)\n");
        return 2;
    }
    if (csr && (fp32ref || a_fp32 || symmetric || gpus != 1 || p2p || nrhs > 0 || spd_n >= 0)) {
        fprintf(stderr, "--csr is fp64 on one GPU from a matrix file (no --fp32-ref, --a-fp32, --symmetric, --gpus, --p2p, --nrhs, --spd)\n");
        return 2;
    }
    const int64_t nsys = nrhs > 0 ? nrhs : 1; /* systems: vectors of nsys * n values */

    /* ---- N ---------------------------------------------------------------- */
    int64_t n = 0;
    if (spd_n > 0) n = spd_n;
    else if (n_opt > 0) n = n_opt;
    else if (dims_path) {
        int64_t d[4];
        if (cgx_text_dims(dims_path, d) != 0) { fprintf(stderr, "%s: cannot read dimensions\n", dims_path); return 1; }
        if (d[0] != d[1]) { printf("%lld and %lld must be same size\n", (long long)d[0], (long long)d[1]); return 1; }
        if (d[2] != d[0] || d[3] != 1) { fprintf(stderr, "%s: b must be %lld x 1\n", dims_path, (long long)d[0]); return 1; }
        n = d[0];
    } else {
        n = cgx_text_count(pos[1]);
        if (n < 0) { printf("Could not open file\n"); fprintf(stderr, "%s: cannot open\n", pos[1]); return 1; }
        if (n % nsys != 0) { fprintf(stderr, "%s: %lld values are not %lld systems\n", pos[1], (long long)n, (long long)nsys); return 1; }
        n /= nsys;
    }
    if (n < 1) { fprintf(stderr, "empty system\n"); return 1; }
    if (csr && n > INT32_MAX) { fprintf(stderr, "--csr: n must be below 2^31\n"); return 1; }
    if (bsr_bs > 0 && n % bsr_bs != 0) {
        fprintf(stderr, "--bsr %lld: n = %lld is not divisible by the block size\n", bsr_bs, (long long)n);
        return 2;
    }
    if (n % gpus != 0) { printf("%lld is not divisible by %d\n", (long long)n, gpus); return 1; } /* parallel_cg.c:88 */

    printf("Computing cg of matrix size : %lld\n", (long long)n * (long long)n); /* serialConjugate.c:58 */
    fflush(stdout);

    const int flags = (fp32ref ? CGX_F32_REF : (CGX_F64 | (symmetric ? CGX_SYMMETRIC : 0))) | (p2p ? CGX_COMM_P2P : 0) |
                      (a_fp32 ? CGX_A_F32 : 0);
    const size_t es = fp32ref ? 4 : 8;           /* b, x */
    const size_t aes = a_fp32 ? 4 : es;          /* A: float with --a-fp32, as initialize() reads it */
    const int a_as_float = fp32ref || a_fp32;
    const size_t vlen = (size_t)(nsys * n); /* values in b and in x */
    void *x = malloc(vlen * es);
    void *A = NULL, *b = NULL;
    /* static: the release thread may still read it while an error path
     * returns from main */
    static release_job rel = {{NULL, NULL, 0}, NULL};
    big_buf Abuf = {NULL, NULL, 0};
    pthread_t freer;
    int freeing = 0;
    /* A's buffers are released on a helper thread AFTER the solve.  Two
     * munmaps of a GiB or more hold the process's mm lock, and a solve that
     * enqueues while they run waits on it: with several row blocks (host-bound:
     * one thread enqueues every block's launches, records and waits) `cg_hip
     * --gpus P --fp32-ref` at N = 4096 / 8192 measured 1-24 ms per solve
     * against 0.7-3.9 ms in a process with nothing to release
     * (profiles/r06_published_mpi_sizes_before.json, r06_multi_solve_latency.jsonl);
     * on one GPU 0.23-0.25 against 0.19-0.20 ms at N = 1024 and 0.33-0.36
     * against 0.30-0.31 at 2048, the same at 4096 / 8192
     * (profiles/r06_cli_release_ab.jsonl).  CGX_CLI_RELEASE=during keeps the
     * release beside the solve (it then overlaps the solve instead of the
     * process's exit). */
    const char *re = getenv("CGX_CLI_RELEASE");
    const int defer_release = !(re && !strcmp(re, "during"));
    const char *se = getenv("CGX_CLI_STREAM");
    const int stream_a = !csr && spd_n <= 0 && !(se && !strcmp(se, "0"));
    if (!x) { fprintf(stderr, "can't allocate memory for vector\n"); return 1; }
    if (spd_n > 0) {
        memset(x, 0, vlen * es);
    } else if (stream_a || csr) {
        b = malloc(vlen * es);
        if (!b) { fprintf(stderr, "can't allocate memory for vector\n"); return 1; }
    } else {
        /* initialize(A), initialize(b), initialize(x0): serialConjugate.c:65-67 */
        if (big_alloc(&Abuf, (size_t)n * (size_t)n * aes) != 0) A = NULL;
        else A = Abuf.p;
        b = malloc(vlen * es);
        if (!A || !b) { fprintf(stderr, "can't allocate memory for vector\n"); return 1; }
    }
    create_job job = {n, gpus, flags, CGX_OK, (int)nrhs, NULL, 0.0, 0.0, csr, -1};
    csr_host csrm = {NULL, NULL, NULL, 0, 0};
    bsr_host bsrm = {NULL, NULL, NULL, 0};
    dia_host diam = {NULL, NULL, 0};
    const double t_start = now_s();
    pthread_t creator;
    const int threaded = pthread_create(&creator, NULL, create_ctx, &job) == 0;
    if (!threaded) create_ctx(&job);
    int read_rc = 0, stream_rc = CGX_OK;
    double t_parsed = 0.0, t_h2d = 0.0;
    if (csr) {
        /* A: indexed once, then parsed and compressed row block by row block
         * while the helper thread starts the HIP runtime; the context is
         * created once the entries are counted */
        cgx_text *text = NULL;
        const int orc = cgx_text_open(pos[0], threads, &text);
        int stopped = 0;
        const int64_t have = orc == 0 ? cgx_text_available(text, &stopped) : -1;
        if (orc != 0) {
            printf("Could not open file\n"); /* serialConjugate.c:103 */
            fprintf(stderr, "%s: cannot open\n", pos[0]);
            read_rc = -1;
        } else if (have < n * n) {
            fprintf(stderr, stopped ? "%s: malformed number\n" : "%s: fewer than %lld numbers\n", pos[0],
                    (long long)(n * n));
            read_rc = stopped ? -3 : -2;
        }
        if (!read_rc) {
            const char *bm = getenv("CGX_CLI_BLOCK_MB");
            const size_t row_bytes = (size_t)n * 8;
            const size_t block_bytes = (size_t)(((bm && atof(bm) > 0) ? atof(bm) : 128.0) * 1048576.0);
            int64_t block_rows = (int64_t)(block_bytes / row_bytes) > 0 ? (int64_t)(block_bytes / row_bytes) : 1;
            if (block_rows > n) block_rows = n;
            if (big_alloc(&Abuf, (size_t)block_rows * row_bytes) != 0) {
                fprintf(stderr, "can't allocate memory for vector\n");
                return 1;
            }
            const int prc = csr_parse(text, n, block_rows, Abuf.p, threads, &csrm, csr_a32);
            if (prc == -9) fprintf(stderr, "can't allocate memory for vector\n");
            else if (prc) fprintf(stderr, prc == -2 ? "%s: fewer than %lld numbers\n" : "%s: malformed number\n", pos[0],
                                  (long long)(n * n));
            read_rc = prc;
            rel.buf = Abuf;
            if (!read_rc && bsr_bs > 0 && bsr_from_csr(&csrm, n, (int)bsr_bs, &bsrm) != 0) {
                fprintf(stderr, "can't allocate memory for vector\n");
                read_rc = -9;
            }
            if (!read_rc && dia && dia_from_csr(&csrm, n, &diam) != 0) {
                fprintf(stderr, "can't allocate memory for vector\n");
                read_rc = -9;
            }
            int64_t bi = 0, bj = 0;
            if (!read_rc && dia_sym && dia_sym_from_dia(&diam, n, &bi, &bj) != 0) {
                fprintf(stderr, "--dia-sym: the matrix is not symmetric: A[i][j] != A[j][i] first at (%lld, %lld), "
                                "mirrored at (%lld, %lld)\n", (long long)bi, (long long)bj, (long long)bj, (long long)bi);
                read_rc = -4;
            }
        }
        t_parsed = now_s();
        if (threaded) pthread_join(creator, NULL); /* before any exit: HIP may be starting up on it */
        if (!read_rc)
            read_rc = read_file(pos[1], (int64_t)vlen, 0, b, threads) || read_file(pos[2], (int64_t)vlen, 0, x, 1);
        rel.text = text;
        if (!read_rc) {
            job.csr_nnz = bsr_bs > 0 ? bsrm.nnzb * bsr_bs * bsr_bs : csrm.nnz; /* blocks are stored whole */
            if (dia && diam.ndiag * n > job.csr_nnz) job.csr_nnz = diam.ndiag * n; /* and so are diagonals */
            create_ctx(&job);
        }
    } else if (stream_a) {
        /* A: indexed once, then parsed and sent row block by row block */
        a_stream st;
        memset(&st, 0, sizeof st);
        const int orc = cgx_text_open(pos[0], threads, &st.text);
        int stopped = 0;
        const int64_t have = orc == 0 ? cgx_text_available(st.text, &stopped) : -1;
        if (orc != 0) {
            printf("Could not open file\n"); /* serialConjugate.c:103 */
            fprintf(stderr, "%s: cannot open\n", pos[0]);
            read_rc = -1;
        } else if (have < n * n) {
            fprintf(stderr, stopped ? "%s: malformed number\n" : "%s: fewer than %lld numbers\n", pos[0],
                    (long long)(n * n));
            read_rc = stopped ? -3 : -2;
        }
        if (!read_rc) {
            const char *rm = getenv("CGX_CLI_RING_MB"), *bm = getenv("CGX_CLI_BLOCK_MB");
            const double ring_mb = (rm && atof(rm) > 0) ? atof(rm) : 1024.0;
            const size_t row_bytes = (size_t)n * aes;
            const size_t block_bytes = (size_t)(((bm && atof(bm) > 0) ? atof(bm) : 128.0) * 1048576.0);
            st.n = n;
            st.es = aes;
            st.block_rows = (int64_t)(block_bytes / row_bytes) > 0 ? (int64_t)(block_bytes / row_bytes) : 1;
            if (st.block_rows > n) st.block_rows = n;
            st.nblocks = (n + st.block_rows - 1) / st.block_rows;
            int64_t slots = (int64_t)(ring_mb * 1048576.0 / ((double)st.block_rows * (double)row_bytes));
            if (slots < 2) slots = 2;
            if (slots > st.nblocks) slots = st.nblocks;
            st.nslots = (int)slots;
            st.as_float = a_as_float;
            st.threads = threads;
            st.slot_bytes = (size_t)st.block_rows * row_bytes;
            st.filled = calloc((size_t)st.nslots, sizeof(int));
            if (!st.filled || big_alloc(&st.ring, (size_t)st.nslots * st.slot_bytes) != 0) {
                fprintf(stderr, "can't allocate memory for vector\n");
                return 1;
            }
            pthread_mutex_init(&st.mu, NULL);
            pthread_cond_init(&st.cv, NULL);
            st.creator = creator;
            st.creator_threaded = threaded;
            st.job = &job;
            pthread_t copier;
            const int copy_threaded = pthread_create(&copier, NULL, stream_copy, &st) == 0;
            if (copy_threaded) {
                const int prc = stream_parse(&st);
                if (prc) {
                    fprintf(stderr, prc == -2 ? "%s: fewer than %lld numbers\n" : "%s: malformed number\n", pos[0],
                            (long long)(n * n));
                    read_rc = prc;
                }
                t_parsed = now_s();
                pthread_join(copier, NULL); /* also joined the creator */
                stream_rc = st.rc;
            } else {
                read_rc = -1;
                if (threaded) pthread_join(creator, NULL);
            }
            t_h2d = st.t_last_h2d;
            rel.buf = st.ring;  /* released after the b and x0 reads */
            free(st.filled);
        } else if (threaded) {
            pthread_join(creator, NULL);
        }
        if (!read_rc)
            read_rc = read_file(pos[1], (int64_t)vlen, fp32ref, b, threads) || read_file(pos[2], (int64_t)vlen, fp32ref, x, 1);
        rel.text = st.text;
        if (!defer_release) {
            if (pthread_create(&freer, NULL, release_buf, &rel) == 0) freeing = 1;
            else release_buf(&rel);
        }
    } else {
        read_rc = spd_n > 0 ? 0
                            : (read_file(pos[0], n * n, a_as_float, A, threads) ||
                               read_file(pos[1], (int64_t)vlen, fp32ref, b, threads) ||
                               read_file(pos[2], (int64_t)vlen, fp32ref, x, 1));
        t_parsed = now_s();
        if (threaded) pthread_join(creator, NULL);  /* before any exit: HIP may be starting up on it */
    }
    const double t_read = now_s();
    if (read_rc) {
        if (job.ctx) cgx_destroy(job.ctx);
        return 1;
    }
    cgx_ctx *ctx = job.ctx;
    int rc = job.rc;
    if (rc != CGX_OK) return die_cgx(rc, "cgx_create");
    if (stream_rc != CGX_OK) return die_cgx(stream_rc, "cgx_set_rows");

    double t_dist0 = stream_a ? t_parsed : now_s(), t_dist1;
    if (spd_n > 0) {
        rc = cgx_generate_spd(ctx, seed);
        t_dist1 = now_s();
        if (rc != CGX_OK) return die_cgx(rc, "cgx_generate_spd");
    } else if (csr) {
        rc = dia_sym    ? cgx_set_dia_sym(ctx, diam.ndiag, diam.offsets, diam.data, n)
             : dia      ? cgx_set_dia(ctx, diam.ndiag, diam.offsets, diam.data, n)
             : bsr_bs > 0 ? cgx_set_bsr(ctx, (int)bsr_bs, bsrm.brow_ptr, bsrm.bcol_idx, bsrm.values)
             : csr_a32  ? cgx_set_csr_f32(ctx, csrm.row_ptr, csrm.col_idx, (const float *)csrm.values)
                        : cgx_set_csr(ctx, csrm.row_ptr, csrm.col_idx, (const double *)csrm.values);
        if (rc != CGX_OK) return die_cgx(rc, dia_sym ? "cgx_set_dia_sym" : dia ? "cgx_set_dia" : bsr_bs > 0 ? "cgx_set_bsr" : csr_a32 ? "cgx_set_csr_f32" : "cgx_set_csr");
        if (jacobi) { /* 1 / diag(A) from the uploaded matrix; a diagonal it refuses ends the run */
            rc = cgx_set_precond(ctx, CGX_PC_JACOBI);
            if (rc != CGX_OK) return die_cgx(rc, "cgx_set_precond");
        }
        if (block_bs > 0) { /* the diagonal blocks of the uploaded matrix; one it cannot invert ends the run */
            rc = cgx_set_precond_block(ctx, (int)block_bs);
            if (rc != CGX_OK) return die_cgx(rc, "cgx_set_precond_block");
        }
        rc = cgx_set_rows(ctx, 0, n, NULL, n, b, x);
        t_dist1 = now_s();
        free(b);
        free(csrm.row_ptr);
        free(csrm.col_idx);
        free(csrm.values);
        free(bsrm.brow_ptr);
        free(bsrm.bcol_idx);
        free(bsrm.values);
        free(diam.offsets);
        free(diam.data);
        if (rc != CGX_OK) return die_cgx(rc, "cgx_set_rows");
    } else if (stream_a) {
        /* A is on the device; b and x0 (MPI_Bcast / MPI_Scatter of the vectors) */
        rc = cgx_set_rows(ctx, 0, n, NULL, n, b, x);
        t_dist1 = now_s();
        free(b);
        if (rc != CGX_OK) return die_cgx(rc, "cgx_set_rows");
    } else {
        /* MPI_Bcast(x0) + MPI_Scatter(A, b): parallel_cg.c:109-117 */
        rc = cgx_set_system(ctx, A, b, x);
        t_dist1 = now_s();
        /* A is no longer needed: release it on a helper thread while the
         * solve runs (unmapping 268 MB took 16-30 ms on the critical path) */
        rel.buf = Abuf;
        if (!defer_release) {
            if (pthread_create(&freer, NULL, release_buf, &rel) == 0) freeing = 1;
            else release_buf(&rel);
        }
        free(b);
        if (rc != CGX_OK) return die_cgx(rc, "cgx_set_system");
    }

    const double t_freed = now_s();
    cgx_stats st;
    const double t_solve0 = now_s();
    rc = cgx_solve(ctx, NULL, eps, max_iter, &st);
    const double t_solve1 = now_s();
    if (rc != CGX_OK) return die_cgx(rc, "cgx_solve");
    rc = cgx_get_x(ctx, x);
    if (rc != CGX_OK) return die_cgx(rc, "cgx_get_x");
    const double t_x = now_s();
    if (defer_release) {
        if (pthread_create(&freer, NULL, release_buf, &rel) == 0) freeing = 1;
        else release_buf(&rel);
    }

    if (gpus > 1) {
        printf("cg method execution time in seconds: %f\n", st.solve_ms / 1e3);
        printf("%s data distribution time in seconds: %f\n", p2p ? "p2p" : "collective", t_dist1 - t_dist0);
        printf("clock execution time in seconds: %f\n", now_s() - t_prog0);
    } else {
        printf("average clock execution time in seconds: %f\n", st.solve_ms / 1e3);
    }
    if (stats)
        printf("iterations: %lld converged: %d residual_norm: %.6e\n", (long long)st.iterations, st.converged,
               st.rr >= 0 ? __builtin_sqrt(st.rr) : -1.0);
    if (stats && csr) printf("nnz: %lld\n", (long long)csrm.nnz);
    if (stats && bsr_bs > 0) printf("nnzb: %lld\n", (long long)bsrm.nnzb);
    if (stats && dia) printf("ndiag: %lld\n", (long long)diam.ndiag);
    if (stats && csr_a32) printf("values: float\n");
    if (stats && jacobi) printf("precond: jacobi\n");
    if (stats && block_bs > 0) printf("precond: block-jacobi %lld\n", block_bs);
    if (stats && nrhs > 0)
        for (int j = 0; j < (int)nrhs; ++j) {
            cgx_stats sj;
            rc = cgx_get_stats_rhs(ctx, j, &sj);
            if (rc != CGX_OK) return die_cgx(rc, "cgx_get_stats_rhs");
            printf("system %d iterations: %lld converged: %d residual_norm: %.6e\n", j, (long long)sj.iterations,
                   sj.converged, sj.rr >= 0 ? __builtin_sqrt(sj.rr) : -1.0);
        }
    if (print_x) {
        for (int64_t i = 0; i < (int64_t)vlen; ++i) {
            if (fp32ref) printf("%.9g\n", (double)((float *)x)[i]);
            else printf("%.17g\n", ((double *)x)[i]);
        }
    }
    fflush(stdout);
    const double t_printed = now_s();
    const char *fx = getenv("CGX_CLI_FAST_EXIT");
    const int fast_exit = !(fx && !strcmp(fx, "0"));
    if (!fast_exit) {
        if (freeing) pthread_join(freer, NULL);
        free(x);
        cgx_destroy(ctx);
    }
    if (getenv("CGX_CLI_TIMES")) /* phase breakdown, seconds since program start */
        fprintf(stderr,
                "{\"setup_s\": %.6f, \"read_s\": %.6f, \"hip_runtime_s\": %.6f, \"create_s\": %.6f, \"distribute_s\": %.6f, "
                "\"solve_s\": %.6f, \"to_x_s\": %.6f, \"printed_s\": %.6f, \"teardown_s\": %.6f, \"fast_exit\": %d, "
                "\"dist_start_s\": %.6f, \"solve_call_s\": %.6f, \"free_s\": %.6f, \"get_x_s\": %.6f, "
                "\"streamed\": %d, \"a_parsed_s\": %.6f, \"a_on_device_s\": %.6f}\n",
                t_start - t_prog0, t_read - t_start, job.t_rt - t_start, job.t_done - t_start, t_dist1 - t_dist0, st.solve_ms / 1e3,
                t_x - t_prog0, t_printed - t_prog0, now_s() - t_printed, fast_exit, t_dist0 - t_start, t_solve1 - t_solve0, t_freed - t_dist1, t_x - t_solve1,
                stream_a, t_parsed > 0 ? t_parsed - t_start : 0.0, t_h2d > 0 ? t_h2d - t_start : 0.0);
    if (fast_exit) {
        /* Every result is written and flushed.  The process ends here without
         * freeing the device/pinned buffers or running the HIP runtime's exit
         * teardown: the kernel driver reclaims both at process exit.  Flush
         * to exit: 29 ms against 71 ms with the teardown at N=8192
         * (CGX_CLI_FAST_EXIT=0 keeps it). */
        fflush(stderr);
        _exit(0);
    }
    return 0;
}
