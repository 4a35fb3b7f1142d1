/*
 * cgx.h -- C ABI of the MI355X-native conjugate-gradient hot path (libcgx.so).
 *
 * This is the drop-in boundary for the reference's CG loop
 * (mawunyega/conjugate_gradient).  The reference has no library API of its
 * own: its solvers are self-contained C programs whose functions are
 *
 *   void  matVec(float *out, float *A, float *x [, int local_row]);
 *         serialConjugate.c:109-120, parallel_cg.c:172-184
 *   float vecVec(float *v1, float *v2 [, int local_row]);
 *         serialConjugate.c:145-155, parallel_cg.c:211-221
 *   void  residual(float *out, float *b, float *Ax [, int]);      :124-131
 *   void  scalarVec / vecAdd / vecSub(...)                          :135-177
 *   void  conjugrad(float *A, float *b, float *x
 *                   [, int local_row, int rank, int P]);
 *         serialConjugate.c:180-259, parallel_cg.c:248-345
 *   MPI_Bcast / MPI_Scatter distribution        parallel_cg.c:109-117
 *   MPI_Allgather(p) + 2x MPI_Allreduce(SUM)     parallel_cg.c:287-313
 *
 * and this header maps each of them to an entry point (see INTEGRATION.md for
 * the function-by-function table and the ctypes / C bindings a maintainer
 * adds).  Conventions:
 *   - plain C types only: pointers, sizes, int status codes; nothing aborts;
 *   - host arrays are caller-owned; device buffers, streams, events and RCCL
 *     communicators are owned by the context;
 *   - a context is not thread-safe; one host thread drives it;
 *   - x is in/out exactly like conjugrad's vectorX (x0 in, solution out).
 *
 * Numerics (flags):
 *   CGX_F64      (default) double data and arithmetic; the fp64 reading of
 *                conjgrad.m.  Dots are deterministic fixed-order reductions.
 *                Precondition: A is finite (with x0 = 0 the initial A x0 is
 *                skipped as exactly zero; an Inf/NaN in A would have made it NaN).
 *   CGX_F32_REF  float data, serialConjugate.c's operation order: sequential
 *                fp32 accumulation per row and per dot, no FMA contraction.
 *                Produces the reference's x bit for bit: serialConjugate.c on
 *                one shard; parallel_cg.c on P row blocks (per-rank partials
 *                combined in MPICH 3.3's MPI_Allreduce order, recursive
 *                doubling); point-to-point_cg.c with CGX_COMM_P2P (rank-order
 *                allSum).  Pinned by mpiexec runs of the unmodified programs
 *                (tests/golden/mpi/).
 *   CGX_A_F32    A stored as float, everything else double: the fp64 solve of
 *                the float matrix the reference's input paths hold
 *                (fscanf("%f"), float *A, MPI_FLOAT) at half the matVec bytes.
 *                - A lives on the device as float, pitch cgx_info.lda floats
 *                  (n rounded up to 256), zero padded.  b, x, r, p, Ap and
 *                  every scalar are double; cgx_info.elem_bytes stays 8 and
 *                  cgx_info.flags carries CGX_A_F32.
 *                - Each a_ij is widened to double inside the kernel (exact)
 *                  and multiplied by p_j with an fp64 FMA; there is no fp32
 *                  arithmetic anywhere.
 *                - Row sums and the fused p.Ap are deterministic fixed-order
 *                  sums, bit-identical for every (R, U, load policy) plan of
 *                  the kernel.  The order differs from k_matvec_f64's:
 *                  results agree with CGX_F64 on the same values to fp64
 *                  rounding (the CGX_SYMMETRIC contract).
 *                - Host side: A_rows / A of cgx_set_rows, cgx_set_system and
 *                  cgx_conjugrad are `const float *` and lda_host counts
 *                  floats; b and x stay double.
 *                - cgx_generate_spd stores (float) of the value the fp64
 *                  generator computes for A_ij (round to nearest); b as in
 *                  fp64 mode.
 *                - One GPU (cgx_create), resident row-major A, optionally
 *                  CGX_TIMING.  CGX_ERR_ARG with CGX_F32_REF, CGX_SYMMETRIC,
 *                  CGX_HOST_STREAM, CGX_PHASES, cgx_create_multi,
 *                  cgx_create_rank and the Poisson constructors.
 *
 * Several right-hand sides (cgx_create_nrhs): nrhs systems A x_j = b_j on one
 * matrix, solved together.  The reference runs conjugrad once per vectorb.txt
 * and streams all of A on every iteration of every run; here one pass over A
 * per iteration multiplies the p vectors of all nrhs systems.
 *   - Batched CG, not block CG: the systems share only the read of A.  Each
 *     has its own alpha, beta and stopping point, and each column's numerics
 *     are those of a one-system CGX_F64 solve (row sums of A p_j bit for bit
 *     cgx_matvec's; dots deterministic fixed-order sums per column).
 *   - Stopping is per column, decided on the device: when sqrt(r_j.r_j) < eps
 *     at iteration k, x_j gets that iteration's update, p_j is left (the
 *     reference's break, serialConjugate.c:235-238), and column j is frozen:
 *     no kernel writes x_j, r_j, p_j or its scalars again.  The solve ends
 *     when every column has stopped (or at the count).
 *   - Host layout: wherever a one-system context takes n values of b or x,
 *     an nrhs context takes nrhs * n, system after system: b[j*n + i] is
 *     entry i of system j (nrhs of the reference's vectors, one after the
 *     other).  cgx_set_rows: b_rows / x_rows hold nrhs blocks of nrows values.
 *   - cgx_generate_spd(seed): A as a one-system context's; b_j is the b that
 *     seed + j gives (column 0 is the one-system context's system); x0 = 0.
 *   - cgx_get_stats: iterations = the largest column count, converged = every
 *     column converged, rr = the largest final r.r; cgx_get_stats_rhs gives
 *     column j's.  cgx_residual_norm is CGX_ERR_ARG (cgx_residual_norms).
 *   - cgx_set_matvec_plan accepts exactly the instantiated (rows per wave,
 *     chunks in flight) of k_matvec_nrhs_f64 for the context's width (nrhs
 *     rounded up to 2, 4 or 8): width 2: (2,4) (4,2) (4,4) (8,2); 4: (4,2)
 *     (4,4) (8,2); 8: (4,1) (4,2); load policy 2 or 8.
 *   - One GPU, CGX_F64, A resident row-major, optionally CGX_TIMING; every
 *     other flag bit is CGX_ERR_ARG.  No creation warm-up.
 *
 * Sparse A (cgx_create_csr): a general sparse SPD matrix in CSR storage, the
 * matrix CG is mostly used on; the reference has none (it holds every A
 * dense).  One GPU, fp64.
 *   - Storage: row_ptr is int64_t[n + 1] (the entry count may pass 2^31),
 *     col_idx int32_t[nnz] (so n < 2^31), values double[nnz]; row i owns the
 *     entries [row_ptr[i], row_ptr[i+1]).
 *   - Entries are taken in stored order: columns need not be sorted, and a
 *     duplicate column is two terms of the sum.  An empty row gives +0.0.
 *   - Summation order (k_csr_mult_f64, T lanes per row, T = 2 .. 64): with
 *     s = row_ptr[i], sub-lane l starts from +0.0 and adds entries s+l,
 *     s+l+T, s+l+2T, ... in that order with one fp64 FMA each; the T partial
 *     sums are combined as v[l] += v[l ^ o] for o = T/2, ..., 1.  A row's sum
 *     depends on T only -- not on the load policy, the grid or the row's place
 *     in a wave; different T agree to fp64 rounding.  The fused p.Ap adds the
 *     blocks' partials in block order: its last bits follow the grid size.
 *   - The structure is checked on the host (cgx_csr_check) by cgx_set_csr
 *     before anything is uploaded; the kernel does not range-check col_idx.
 *     The matrix is not checked for symmetry or definiteness (no mode does).
 *   - The iteration is the three-launch one (matVec with fused p.Ap, r, x/p)
 *     in every host form -- device-gated, CGX_GATED=0, fixed count, in pieces
 *     -- so x is the same bits across them for a given plan.  No two-launch
 *     small-n forms, no creation warm-up.
 *   - Refused: cgx_set_rows / cgx_set_system with a non-NULL A and
 *     cgx_generate_spd (CGX_ERR_ARG); cgx_solve_begin, cgx_solve and
 *     cgx_residual_norm before the first cgx_set_csr (CGX_ERR_STATE); every
 *     flag bit but CGX_TIMING at creation (CGX_ERR_ARG).  b and x go in
 *     through cgx_set_rows (A_rows = NULL), cgx_set_x, cgx_fill.
 *   - cgx_set_matvec_plan: rows_per_wave = 64 / T in {1, 2, 4, 8, 16, 32},
 *     chunks_in_flight = 1, load policy 2 or 8; anything else is CGX_ERR_ARG
 *     and leaves the plan as it was.  cgx_get_info: lda = the vectors' pitch,
 *     elem_bytes = 8, flags carries CGX_CSR_ACTIVE.
 *   - Diagonal preconditioning (cgx_set_precond, cgx_set_precond_diag): the
 *     iteration becomes preconditioned CG with M^-1 = diag(minv), minv the n
 *     positive values 1 / diag(A) (CGX_PC_JACOBI) or the caller's
 *     (CGX_PC_DIAG).  Still three launches per iteration in every host form,
 *     and x the same bits across the forms for a given plan: the SpMV with
 *     p.Ap unchanged; r -= alpha Ap with r.r and r.z from one pass (alpha =
 *     r.z_old / p.Ap, z_i = fl(minv_i r_i), a rounded product, never stored);
 *     x += alpha p and p = z + beta p (beta = r.z_new / r.z_old, z
 *     recomputed).  The solve starts from r = b - A x, p = minv o r.
 *     - Refusals: a context that is not a cgx_create_csr context, an unknown
 *       kind, CGX_PC_DIAG passed to cgx_set_precond, a NULL ctx or pointer:
 *       CGX_ERR_ARG; a call before the first cgx_set_csr: CGX_ERR_STATE.
 *     - A successful call ends a solve in progress, as cgx_set_csr does.
 *     - cgx_set_csr turns preconditioning off (the diagonal belonged to the
 *       old matrix): the caller asks for it again.
 *     - CGX_PC_JACOBI: d_i is the sum, from +0.0 in stored order, of row i's
 *       entries whose column is i (a duplicate is two terms, as in the SpMV);
 *       minv_i = 1.0 / d_i, the correctly rounded fp64 quotient (the bits of
 *       the host's 1.0 / d).  A row with no diagonal entry, or with a d_i
 *       that is not finite or not > 0, fails the call: CGX_ERR_SHAPE naming
 *       the lowest such row and its d_i.  The context then keeps the
 *       preconditioner it had; a later solve gives the bits it gave before.
 *     - The stopping rule and the stats do not change: the loop ends when
 *       sqrt(r.r) < eps (r, not z), cgx_stats.rr is r.r, cgx_residual_norm is
 *       the true residual.
 *     - minv == 1.0 everywhere gives the unpreconditioned x, loop count and
 *       r.r bit for bit on the same plan; so does minv == a power of two
 *       (alpha absorbs the factor, p carries it).
 *     - cgx_get_info: flags carries CGX_PRECOND_ACTIVE while a kind is set.
 *   - Block-Jacobi preconditioning (cgx_set_precond_block,
 *     cgx_set_precond_block_values; kind CGX_PC_BLOCK): M^-1 = W, the inverses
 *     of A's bs x bs diagonal blocks, 2 <= bs <= CGX_MAX_PC_BLOCK, for systems
 *     with bs coupled unknowns per node.  Block k covers rows [k bs,
 *     min(n, (k+1) bs)); nblk = ceil(n / bs); when n % bs != 0 the last block
 *     is t x t with t = n % bs (bs > n: one short block, M = A).  On the host
 *     blocks are nblk * bs * bs doubles, block after block, row-major inside
 *     one; a short block's unused rows and columns are +0.0 on output and
 *     ignored on input.
 *     - Extraction (cgx_csr_diag_blocks, on the device): D_k[i][j] is the sum,
 *       from +0.0 in stored order, of row k bs + i's entries whose column is
 *       k bs + j (a duplicate is two terms); +0.0 where there is none.
 *     - Inversion (cgx_precond_block_invert, on the host, contraction off):
 *       Cholesky D_k = L L^T from the lower triangle only (no symmetry check),
 *       W_k = L^-T L^-1 with the lower triangle computed and mirrored.  A
 *       pivot that is not finite or not > 0 is CGX_ERR_SHAPE naming the
 *       lowest such block, its rows and the pivot.
 *     - cgx_set_precond_block: extract, download, invert, upload (a one-time
 *       cost).  When it fails the context keeps the preconditioner it had and
 *       a later solve gives the bits it gave before; when it succeeds it ends
 *       a solve in progress.  cgx_set_precond_block_values takes the caller's
 *       W after cgx_precond_block_check (every used entry finite, every used
 *       diagonal entry > 0; CGX_ERR_SHAPE names W[block][i][j], nothing
 *       changes); whether those blocks are symmetric and positive definite is
 *       the caller's business -- CG needs an SPD M.  cgx_set_csr turns the kind
 *       off, as every kind.
 *     - Order of z = W r (the contract): for row i of block k, with j over the
 *       block's rows in ascending order, z_i = fl(W[i][0] r_0), then z_i =
 *       fma(W[i][j], r_j, z_i) for j = 1, ...  So blocks whose off-diagonal
 *       entries are 0 give CGX_PC_DIAG's z bit for bit.  z is stored (one more
 *       n-vector on the context): the r update forms it from the new r it
 *       holds, the x/p update reads it.  r.r and r.z are fixed-order sums in
 *       an order of their own (not the diagonal kernels'): deterministic for a
 *       given (n, bs).
 *     - The iteration is otherwise the diagonal kinds': three launches in every
 *       host form and x, the loop count and r.r the same bits across them for
 *       a given plan; alpha = r.z_old / p.Ap, beta = r.z_new / r.z_old, the
 *       stop on sqrt(r.r) < eps; stats and cgx_residual_norm unchanged.
 *     - Refusals.  CGX_ERR_ARG: a context that is not a plain cgx_create_csr
 *       context (a cgx_create_csr_nrhs context included), bs outside the range
 *       (bs = 1 is CGX_PC_JACOBI), a NULL argument; cgx_set_precond(ctx,
 *       CGX_PC_BLOCK) -- the kind has its own entry points, as CGX_PC_DIAG.
 *       CGX_ERR_STATE: a call before the first cgx_set_csr;
 *       cgx_get_precond_block while the kind is not CGX_PC_BLOCK;
 *       cgx_get_precond_diag while it is.
 *     - cgx_get_precond reports CGX_PC_BLOCK for both ways in; cgx_get_info
 *       carries CGX_PRECOND_ACTIVE.
 *     - Pinned by tests/test_gpu_pcg_probe.py (reference and bars in
 *       tests/_pcg_probe.py) for every bs, every short last block t = 0 ..
 *       bs - 1 with NaN in its unused slots, an unsymmetric W, and the
 *       diagonal kinds at the edges of their pair loop: after each of three
 *       fixed iterations from a rough x0 every element of x agrees with the
 *       same recurrence in extended precision to 100 x the spread between
 *       fp64 summation orders (at most 1.5e-11 of the terms added into that
 *       element).
 *   - Several right-hand sides (cgx_create_csr_nrhs): nrhs (1..CGX_MAX_NRHS)
 *     systems A x_j = b_j on one CSR matrix, the CSR arrays read once per
 *     iteration (k_csr_mult_f64).  The context is a cgx_create_csr context's
 *     matrix with a cgx_create_nrhs context's vectors, scalars and loop.
 *     - Order per column: exactly the one above at the same T.  Column j of a
 *       product is cgx_spmv_csr's result on column j bit for bit; it does not
 *       depend on the width K (nrhs rounded up to 2, 4 or 8), the load policy
 *       or the grid.
 *     - Layout: b and x hold nrhs * n values, system after system; on the
 *       device column j starts at j * lda doubles (cgx_info.lda).  Values and
 *       col_idx are loaded once per entry and multiplied by K gathered vector
 *       elements; columns nrhs..K-1 read column 0 again and are not stored.
 *     - Freeze and stats as "Several right-hand sides" above: each column has
 *       its own alpha, beta and stopping point, a stopped column is frozen,
 *       cgx_get_stats / cgx_get_stats_rhs / cgx_residual_norms report as on a
 *       cgx_create_nrhs context.  Three launches per iteration in every host
 *       form; x the same bits across the forms for a given plan.
 *     - Plans: cgx_set_matvec_plan as on a cgx_create_csr context
 *       (rows_per_wave = 64 / T, chunks_in_flight = 1, policy 2 or 8); the
 *       default T follows the mean row length.  cgx_set_csr plans again
 *       unless the caller chose a plan.
 *     - Refusals: at creation nrhs outside [1, CGX_MAX_NRHS], n < 1,
 *       n >= 2^31, nnz < 0 or any flag bit but CGX_TIMING (CGX_ERR_ARG, *ctx
 *       NULL, before the device is touched); cgx_generate_spd, a non-NULL A,
 *       cgx_residual_norm, cgx_set_precond, cgx_set_precond_diag and
 *       cgx_set_precond_block[_values]
 *       (CGX_ERR_ARG: batched CG has no preconditioned update kernels);
 *       cgx_solve_begin, cgx_solve and cgx_residual_norms before the first
 *       cgx_set_csr (CGX_ERR_STATE).
 *   - Float-stored values (cgx_set_csr_f32, on a cgx_create_csr or
 *     cgx_create_csr_nrhs context): the values go up and stay on the device as
 *     float[nnz], which is what the reference holds on every input path; an
 *     entry then streams 8 bytes per product in place of 12.  There is no fp32
 *     arithmetic: every kernel widens a value with (double), which is exact
 *     (denormals included), and then does the double-valued kernel's fp64
 *     operations in the same order.
 *     - The contract: a float-valued context gives, bit for bit, what a
 *       double-valued context gives on (double)values[e] -- the row sums of the
 *       SpMV and the SpMM at the same T, the fused p.Ap on the same grid,
 *       1 / diag(A), the diagonal blocks and their inverses, and so x, the
 *       loop count and r.r in every host form, with every preconditioner kind.
 *     - The context is float-valued until the next cgx_set_csr (double-valued
 *       again) or cgx_set_csr_f32.  cgx_set_csr_f32 is cgx_set_csr otherwise:
 *       the same checks in the same order and the same refusals, nothing
 *       uploaded when one fails (the earlier matrix, its value type and its
 *       preconditioner stay), a solve in progress ended, preconditioning off,
 *       and a new default plan unless the caller chose one (the default T rule
 *       is the same for both value types).
 *     - cgx_get_info: flags carries CGX_A_F32 (reported) while the context is
 *       float-valued; elem_bytes stays 8.  CGX_A_F32 at cgx_create_csr stays
 *       refused: the value type comes with the matrix, not with the context.
 *     - The allocation is not halved: the floats live in the context's value
 *       buffer, which has room for nnz doubles.  A constructor that allocates
 *       4 bytes per entry is not built.
 *     - Kernel-level: cgx_spmv_csr_f32, cgx_spmm_csr_f32.  cgx_csr_diag_blocks
 *       takes double values only.
 *   - Several row blocks (cgx_create_csr_multi): one process, nshards
 *     contiguous equal row blocks of n / nshards rows on devices[0 ..
 *     nshards - 1] (a device may repeat), as cgx_create_multi makes them; each
 *     block owns the CSR arrays of its rows with room for nnz_block entries.
 *     - Refused before any device is touched (*ctx NULL): n % nshards != 0
 *       (CGX_ERR_SHAPE); nshards outside [1, 32], n < 1, n >= 2^31,
 *       nnz_block < 0, any flag bit but CGX_TIMING, a NULL pointer
 *       (CGX_ERR_ARG).
 *     - cgx_set_csr / cgx_set_csr_f32 take the whole matrix's host arrays
 *       (row_ptr[n + 1], global col_idx, values) and run the checks above in
 *       the same order (the room is per block, so the total is not compared
 *       with it); then a block with more than nnz_block entries is
 *       CGX_ERR_SHAPE naming the block and its count.  Nothing is uploaded
 *       and no list is replaced when a check fails: the earlier matrix, its
 *       value type and its lists stay, and a later solve gives the bits it
 *       gave before.  Block i receives its rows' row_ptr rebased to start at
 *       0 and its slices of col_idx (still global columns) and values.  The
 *       call ends a solve in progress.
 *     - One T for the context: by default the T plan_spmv_csr chooses for
 *       the whole matrix (n, all its entries), which is what a cgx_create_csr
 *       context chooses; each block's grid comes from its own rows.
 *       cgx_set_matvec_plan applies to every block under the rules above.
 *     - The exchange.  A block needs only the entries of p that its col_idx
 *       names outside its own rows.  cgx_set_csr builds, on the host, for
 *       every pair (d, q != d) the ascending distinct offsets into block q
 *       that block d's rows name (one pass over the block's col_idx with a
 *       mark array, then a scan; cgx_csr_halo_counts / cgx_csr_halo_list run
 *       the same builder without a GPU), and one pull kernel per consuming
 *       block (k_gather_indexed, after the producers' events) moves exactly
 *       those entries into the block's full-length p each iteration; the
 *       same lists serve the exchange of x at the start of a solve from
 *       x0 != 0 and in cgx_residual_norm.  A pair whose list is the whole
 *       slice (a dense row or column) takes the contiguous path, an empty
 *       list moves nothing.  Positions of the full-length p outside the own
 *       slice and the lists are never written, and no kernel reads them.
 *       CGX_CSR_XCHG=full runs the whole-slice pull kernel of
 *       cgx_create_multi instead, CGX_LOCAL_XCHG=copy its peer copies; the
 *       three forms give the same x bit for bit, and cgx_get_info carries
 *       CGX_CSR_HALO_ACTIVE only under the first.
 *     - Memory: the full-length p costs n doubles on every block (134 MB per
 *       block at 16.8 M rows), whatever the lists' lengths.
 *     - Bits: given the same p, a block's rows of A p are the one-GPU
 *       kernel's row sums bit for bit at the same T, float-stored values
 *       included; p.Ap and r.r are each block's fixed-order partial sums
 *       combined in block order.  So x agrees with a one-GPU solve to fp64
 *       rounding and is deterministic for a partition and a plan: the same
 *       bits in every host form (device-gated, CGX_GATED=0, fixed count, in
 *       pieces), under every exchange form, with CGX_LOCAL_FUSE=0 / 1 and
 *       CGX_LOCAL_THREADS=0 / 1, on distinct devices as on one device
 *       repeated.  With nshards == 1 the context gives cgx_create_csr's x,
 *       loop count and r.r bit for bit.
 *     - The iteration stays the three-launch one (no two-launch forms, no
 *       creation warm-up); the dense overlap does not apply
 *       (cgx_get_overlap_info: CGX_OV_NA).
 *     - Refused (CGX_ERR_ARG) whatever nshards is: cgx_set_precond,
 *       cgx_set_precond_diag, cgx_set_precond_block[_values] (the PCG kernels
 *       read their scalars from one block's slots), cgx_generate_spd, a
 *       non-NULL A.  cgx_solve_begin, cgx_solve, cgx_residual_norm and
 *       cgx_get_csr_halo before the first cgx_set_csr: CGX_ERR_STATE.
 *       cgx_create_csr_nrhs stays one GPU.
 *   - Block storage (cgx_set_bsr, on a plain cgx_create_csr context): systems
 *     with bs coupled unknowns per node -- the ones cgx_set_precond_block was
 *     built for -- are block matrices, every nonzero a dense bs x bs block.
 *     Held as BSR an entry streams 8 + 4 / bs^2 bytes in place of CSR's 12 and
 *     a block reads its bs vector elements as one contiguous piece in place of
 *     bs^2 gathers.  2 <= bs <= CGX_MAX_BSR_BLOCK; bs = 1 is cgx_set_csr.
 *     - Storage (scipy's bsr_matrix): brow_ptr is int64_t[nb + 1], bcol_idx
 *       int32_t[nnzb], values double[nnzb * bs * bs], block after block,
 *       row-major inside a block; n = nb * bs.  Block row I owns the blocks
 *       [brow_ptr[I], brow_ptr[I+1]) in stored order: block columns need not
 *       be sorted, a duplicate block column is two terms, a stored zero is a
 *       term.
 *     - Summation order (k_bsr_mult_f64, T lanes per block row, T = 2 .. 64).
 *       For scalar row I bs + i, with s = brow_ptr[I]: sub-lane l starts from
 *       +0.0 and, for each of its blocks s+l, s+l+T, ... in that order and
 *       j = 0 .. bs-1 ascending inside a block in block column c, does
 *       acc_i = fma(B[i][j], v[c bs + j], acc_i); the T partial sums are
 *       combined as v[l] += v[l ^ o] for o = T/2, ..., 1.  A row's sum depends
 *       on (bs, T) only -- not on the load policy, the grid, the trips in
 *       flight, the row's place in a wave or the device layout of the values;
 *       an empty block row gives bs values of +0.0.  The fused p.Ap: the
 *       storing lane adds its bs rows in ascending order, then as the CSR
 *       kernel's; deterministic for a given (bs, T, grid).
 *     - On the device the values lie in tiles of 64 consecutive blocks,
 *       entry-major inside a tile (entry e of block q at
 *       ((q / 64) bs^2 + e) 64 + q % 64), so a wave's loads are contiguous.
 *       cgx_set_bsr re-lays them once with a kernel into memory of the
 *       library's own (ceil(nnzb / 64) 64 bs^2 doubles, beside the host-layout
 *       copy the preconditioner set-up reads); it is not charged to the
 *       context's capacity.
 *     - cgx_set_bsr checks, in this order: a NULL context or brow_ptr
 *       (CGX_ERR_ARG); not a plain cgx_create_csr context -- cgx_create_csr_nrhs
 *       and cgx_create_csr_multi included, batched and row-block BSR are not
 *       built (CGX_ERR_ARG); bs outside [2, 8] (CGX_ERR_ARG); n % bs != 0
 *       (CGX_ERR_SHAPE); a NULL bcol_idx or values with nnzb > 0
 *       (CGX_ERR_ARG); nnzb bs^2 above the creation-time nnz (CGX_ERR_SHAPE,
 *       both counts named); cgx_bsr_check, cgx_csr_check's rules on the block
 *       structure with nb block columns, the first offence named.  Nothing is
 *       uploaded when one fails: the earlier matrix (CSR or BSR), its value
 *       type, its plan and its preconditioner stay, and a later solve gives
 *       the bits it gave before.
 *     - A successful call ends a solve in progress, turns preconditioning
 *       off, makes a new default plan unless the caller chose one (then T and
 *       the policy are kept), and makes the context block-valued until the
 *       next cgx_set_csr / cgx_set_csr_f32, after which the context gives a
 *       fresh CSR context's bits again.  cgx_get_info: flags carries
 *       CGX_BSR_ACTIVE | CGX_CSR_ACTIVE while the context is block-valued.
 *     - cgx_set_matvec_plan: rows_per_wave = 64 / T counts block rows,
 *       chunks_in_flight = 1, load policy 2 or 8, refusals as on CSR.  The
 *       default T is the largest instantiated T <= the mean blocks per block
 *       row, at least 2, policy 2 (measured at bs = 3 and 4);
 *       CGX_BSMV_PLAN="T=..,nt=..,bpc=.." overrides it.
 *     - The iteration is untouched: the three-launch one in every host form,
 *       x the same bits across them for a given plan; only the matVec (and
 *       cgx_residual_norm's) is the block kernel.
 *     - Preconditioners: cgx_set_precond_diag and
 *       cgx_set_precond_block_values never read the matrix.  CGX_PC_JACOBI and
 *       cgx_set_precond_block(pbs), any pbs in 2..8 and not only pbs == bs,
 *       extract from the BSR arrays and give, bit for bit, the 1 / diag(A) and
 *       the diagonal blocks a double-valued CSR context gives on the expanded
 *       matrix (scalar row I bs + i's entries listed block after block in
 *       stored order, j ascending inside a block); the failures are CSR's.
 *     - Not built: float-stored BSR values, several right-hand sides, several
 *       row blocks, bs = 1, a rectangular block shape.
 *   - Diagonal storage (cgx_set_dia, on a plain cgx_create_csr context):
 *     structured grids with variable coefficients, 5-, 7- and 27-point stencils
 *     and banded systems are a handful of diagonals.  Held by diagonals a matrix
 *     has no column indices and no gathers: an entry streams 8 bytes in place
 *     of CSR's 12, a row 8 ndiag + 16 in place of 12 L + 24.
 *     - Storage (scipy's dia_matrix, square): offsets is int32_t[ndiag], data
 *       double[ndiag * ld] with ld >= n; data[k * ld + j] is
 *       A[j - offsets[k]][j] -- the slot is indexed by the column.  Row i reads
 *       data[k * ld + i + o] and v[i + o], o = offsets[k], where
 *       0 <= i + o < n.  Slots outside that range are never read, on the host
 *       or on the device, and may hold NaN.  Diagonals are taken in stored
 *       order and need not be sorted, a duplicate offset is two terms, a stored
 *       zero is a term.  ndiag = 0 is the zero matrix (the pointers may be
 *       NULL).
 *     - Summation order (k_dia_mult_f64).  Row i starts from +0.0 and, for
 *       k = 0 .. ndiag-1 in stored order where 0 <= i + offsets[k] < n, does
 *       acc = fma(data[k][i + o], v[i + o], acc): one accumulator per row, no
 *       cross-lane combine.  A row's sum depends on nothing but the matrix and
 *       v -- not on the rows per lane, the diagonals in flight, the load
 *       policy, the grid or the device pitch; a row no diagonal reaches gives
 *       +0.0.  The fused p.Ap goes the CSR kernel's way; deterministic for a
 *       given rows per lane and grid.
 *     - cgx_dia_check (host only): n < 1, ndiag < 0 or NULL offsets with
 *       ndiag > 0 is CGX_ERR_ARG; an offset <= -n or >= n is CGX_ERR_SHAPE,
 *       the first such k and its value named.
 *     - cgx_set_dia checks, in this order: a NULL context (CGX_ERR_ARG); not a
 *       plain cgx_create_csr context -- cgx_create_csr_nrhs and
 *       cgx_create_csr_multi included, batched and row-block DIA are not built
 *       (CGX_ERR_ARG); ndiag < 0, or NULL offsets / data with ndiag > 0
 *       (CGX_ERR_ARG); ld < n (CGX_ERR_SHAPE); ndiag n above the creation-time
 *       nnz (CGX_ERR_SHAPE, both counts named; the padding of the device pitch
 *       is not charged); cgx_dia_check.  Nothing is uploaded when one fails:
 *       the earlier matrix (CSR, BSR or DIA), its value type, its plan and its
 *       preconditioner stay, and a later solve gives the bits it gave before.
 *     - A successful call ends a solve in progress, turns preconditioning off,
 *       makes a new default plan unless the caller chose one on a
 *       diagonal-valued context already, and makes the context diagonal-valued
 *       until the next cgx_set_csr / cgx_set_csr_f32 / cgx_set_bsr, after which
 *       the context gives a fresh context's bits again (and a default plan).
 *       cgx_get_info: flags carries CGX_DIA_ACTIVE | CGX_CSR_ACTIVE, never
 *       CGX_BSR_ACTIVE with it.  On the device the diagonals lie at an even
 *       pitch, in the context's own values where they fit and otherwise (an
 *       odd n at full capacity) in memory of the library's own.
 *     - cgx_set_matvec_plan: rows_per_wave = 64 R in {64, 128} (R rows per
 *       lane), chunks_in_flight = U in {1, 2, 4, 8} diagonals in flight, load
 *       policy 2 or 8; anything else is CGX_ERR_ARG and the plan stays.
 *       The default is R = 1, U = 1, policy 8 (measured at 5 and 65 diagonals,
 *       DESIGN.md s3); CGX_DIA_PLAN="R=..,U=..,nt=..,bpc=.." (R = 1 or 2)
 *       overrides it.
 *     - The iteration is untouched: the three-launch one in every host form,
 *       x the same bits across them for a given plan; only the matVec (and
 *       cgx_residual_norm's) is the diagonal kernel.
 *     - Preconditioners: cgx_set_precond_diag and
 *       cgx_set_precond_block_values never read the matrix.  CGX_PC_JACOBI and
 *       cgx_set_precond_block(pbs), any pbs in 2..8, extract from the
 *       diagonals and give, bit for bit, the 1 / diag(A) and the diagonal
 *       blocks a double-valued CSR context gives on the expanded matrix (row
 *       i's entries listed diagonal after diagonal in stored order, in-range
 *       terms only, stored zeros included); the failures are CSR's.
 *     - Not built: float-stored diagonals, several right-hand sides, several
 *       row blocks, rectangular matrices.  One-sided storage of a symmetric A
 *       is the next paragraph.
 *   - One-sided diagonal storage (cgx_set_dia_sym, on a plain cgx_create_csr
 *     context): CG needs a symmetric A, so the diagonals of triu(A) say
 *     everything.  Each stored value is used twice, o rows apart: the byte
 *     model is 8 ndiag_stored + 16 per row (5-point Poisson: 40 in place of
 *     56; 65 diagonals: 280 in place of 536) where the second use finds its
 *     line on the die, and the matrix needs half the memory.  Symmetry
 *     cannot be checked -- only one triangle is given: what is multiplied is
 *     the symmetric matrix whose upper triangle the arrays hold.
 *     - Storage (scipy's dia_matrix of triu(A)): offsets is int32_t[ndiag]
 *       with 0 <= offsets[k] < n, data double[ndiag * ld] with ld >= n;
 *       data[k * ld + j] = A[j - o][j] for j in [o, n), o = offsets[k].  Slots
 *       j < o and j >= n are never read, on the host or on the device, and
 *       may hold NaN.  The stored diagonal of offset o > 0 also stands for
 *       the diagonal -o: A[j][j - o] = A[j - o][j].  Diagonals are taken in
 *       stored order and need not be sorted, a duplicate offset is two terms,
 *       each with its mirror, a stored zero is a term.  ndiag = 0 is the zero
 *       matrix.
 *     - Summation order (k_dia_sym_mult_f64).  Row i starts from +0.0 and,
 *       for k = 0 .. ndiag-1 in stored order: o = 0 does
 *       acc = fma(data[k][i], v[i], acc); o > 0 does the upper term first,
 *       acc = fma(data[k][i + o], v[i + o], acc) where i + o < n, then the
 *       lower term acc = fma(data[k][i], v[i - o], acc) where i - o >= 0.
 *       One accumulator per row, no cross-lane combine; a row's sum depends
 *       on nothing but the matrix and v.  The expansion: this is, bit for
 *       bit, what k_dia_mult_f64 gives on the full DIA matrix in which every
 *       stored k with o > 0 is two consecutive diagonals, o then -o (the
 *       mirrored one data'[j] = data[k][j + o], j in [0, n - o)) and a
 *       diagonal with o = 0 stays one.  The fused p.Ap is that kernel's on
 *       the expansion at the same rows per lane and grid.
 *     - cgx_dia_sym_check (host only): n < 1, ndiag < 0 or NULL offsets with
 *       ndiag > 0 is CGX_ERR_ARG; an offset < 0 or >= n is CGX_ERR_SHAPE, the
 *       first such k and its value named (a negative one with the reminder
 *       that one-sided storage holds offsets >= 0).
 *     - cgx_set_dia_sym runs cgx_set_dia's checks in cgx_set_dia's order; the
 *       capacity check compares ndiag n, the stored count (not the
 *       expansion's), with the creation-time nnz; cgx_dia_sym_check is last.
 *       Nothing is uploaded when one fails: the earlier matrix (CSR, BSR, DIA
 *       or one-sided), its value type, plan and preconditioner stay.
 *     - A successful call ends a solve in progress, turns preconditioning
 *       off, makes a new default plan unless the caller chose one on a
 *       one-sided context already, and makes the context one-sided until the
 *       next cgx_set_csr / cgx_set_csr_f32 / cgx_set_bsr / cgx_set_dia, after
 *       which the context gives a fresh context's bits.  cgx_get_info: flags
 *       carries CGX_DIA_SYM_ACTIVE | CGX_DIA_ACTIVE | CGX_CSR_ACTIVE.
 *     - cgx_set_matvec_plan: as on a diagonal-valued context (rows_per_wave
 *       64 or 128, chunks_in_flight 1, 2, 4 or 8 stored diagonals, policy 2
 *       or 8 -- of the values' last use; the first use is a default-policy
 *       load).  CGX_DIA_SYM_PLAN="R=..,U=..,nt=..,bpc=.." (R = 1 or 2)
 *       overrides the default.
 *     - The iteration is untouched; only the matVec (and cgx_residual_norm's)
 *       is the one-sided kernel.
 *     - Preconditioners: cgx_set_precond_diag and
 *       cgx_set_precond_block_values never read the matrix.  CGX_PC_JACOBI
 *       (the offset-0 diagonals) and cgx_set_precond_block(pbs), pbs in 2..8
 *       (row r takes, per stored k with o > 0, (r + o, data[k][r + o]) then
 *       (r - o, data[k][r])) give, bit for bit, what a double-valued CSR
 *       context gives on the expansion; the failures are CSR's.
 *     - Not built: float-stored one-sided values, several right-hand sides,
 *       row blocks, one-sided BSR.
 *
 * Multi-GPU: the matrix is split into contiguous row blocks (parallel_cg.c:83,
 * 97-99; n % nranks == 0 as parallel_cg.c:86-90 requires).  Per iteration
 * the p vector is allgathered and the two scalars p.Ap and r.r are
 * allreduced (RCCL over xGMI in rank mode; in the multi-shard mode one pull
 * kernel per consuming row block reads the other blocks' slices / partials
 * through peer pointers).  x stays distributed and is gathered on demand.
 */
#ifndef CGX_H
#define CGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGX_VERSION 101 /* 0.1.1: cgx_overlap_info gained the end-to-end form times; CGX_A_F32 added (a new
                           flag bit: no existing call changes meaning); cgx_create_nrhs and its
                           entry points added (new functions only: no struct changes size, no
                           existing call changes meaning, so the version stays); likewise
                           cgx_create_csr and its entry points, and the reported bit
                           CGX_CSR_ACTIVE; likewise cgx_set_precond and its entry points,
                           and the reported bit CGX_PRECOND_ACTIVE; likewise
                           cgx_create_csr_nrhs and cgx_spmm_csr (new functions only, no new bit);
                           likewise cgx_set_precond_block and its entry points and the kind
                           CGX_PC_BLOCK (new functions only, no new bit); likewise
                           cgx_set_csr_f32, cgx_spmv_csr_f32 and cgx_spmm_csr_f32 (new functions
                           only; CGX_A_F32 is also reported by a float-valued CSR context); likewise
                           cgx_create_csr_multi, cgx_csr_halo_counts, cgx_csr_halo_list,
                           cgx_get_csr_halo and cgx_gather_indexed, and the reported bit
                           CGX_CSR_HALO_ACTIVE; likewise cgx_set_bsr, cgx_bsr_check, cgx_spmv_bsr and
                           cgx_bsr_tile_values, and the reported bit CGX_BSR_ACTIVE; likewise cgx_set_dia,
                           cgx_dia_check and cgx_spmv_dia, and the reported bit CGX_DIA_ACTIVE; likewise
                           cgx_set_dia_sym, cgx_dia_sym_check and cgx_spmv_dia_sym, and the reported bit
                           CGX_DIA_SYM_ACTIVE */

/* ---- status codes (0 = OK, negative = error) --------------------------- */
#define CGX_OK            0
#define CGX_ERR_ARG      -1  /* bad argument / unsupported combination        */
#define CGX_ERR_HIP      -2  /* a HIP runtime call failed                      */
#define CGX_ERR_RCCL     -3  /* an RCCL call failed                            */
#define CGX_ERR_SHAPE    -4  /* n not divisible by ranks, rows out of range   */
#define CGX_ERR_NOMEM    -5  /* device or pinned allocation failed            */
#define CGX_ERR_STATE    -6  /* call out of order (iterate before begin, ...) */
#define CGX_ERR_NODEV    -7  /* no usable GPU                                  */

/* ---- flags ---------------------------------------------------------------- */
#define CGX_F64          0x0   /* double data (default)                        */
#define CGX_F32_REF      0x1   /* float data, bit-exact serialConjugate.c order */
#define CGX_A_F32        0x2   /* float A, double vectors and arithmetic (above) */
#define CGX_DIA_ACTIVE   0x4   /* reported in cgx_info.flags: a cgx_create_csr context that is
                                  diagonal-valued (cgx_set_dia), beside CGX_CSR_ACTIVE */
#define CGX_DIA_SYM_ACTIVE 0x8 /* reported in cgx_info.flags: a diagonal-valued context that holds the
                                  upper diagonals of a symmetric A (cgx_set_dia_sym), beside
                                  CGX_DIA_ACTIVE | CGX_CSR_ACTIVE */
#define CGX_TIMING       0x100 /* time every matVec launch with HIP events      */
#define CGX_NO_OVERLAP   0x400 /* multi-shard dense fp64: do not overlap the p
                                  exchange with the own-column-block matVec
                                  (the allgather, then one matVec launch).
                                  Without it the form is chosen at creation
                                  when every row block is a multiple of 128
                                  rows: the overlap runs only if that whole
                                  form (allgather beside the split matVec),
                                  timed end to end at creation, beats the
                                  plain one by 1 % (cgx_get_overlap_info;
                                  env CGX_OVERLAP=0 / 1: never / always).  Both
                                  forms give the same bits. */
#define CGX_OVERLAP_ACTIVE 0x800 /* reported in cgx_info.flags when it is on */
#define CGX_FUSED_ACTIVE 0x2000 /* reported in cgx_info.flags: a fused
                                   iteration is on -- the Poisson operator's
                                   two-kernel iteration (even m; env
                                   CGX_POISSON_FUSED=0 selects the stencil /
                                   r / x,p three-kernel split), or a small
                                   dense fp64 system on one GPU iterating in
                                   two launches instead of three (n <= 8192;
                                   env CGX_FUSE_P=0 / 1: never / any n);
                                   results are the same bits either way */
#define CGX_COMM_P2P     0x1000 /* point-to-point_cg.c's exchange instead of
                                   collectives: gather to rank 0, then rank 0
                                   sends to every rank (ncclSend/Recv; device
                                   copies through shard 0 in multi-shard mode).
                                   Scalars are summed in rank order (allSum,
                                   point-to-point_cg.c:339-359).  For the
                                   p2p-vs-collective comparison of the report. */
#define CGX_DETERMINISTIC 0x4000 /* rank mode, fp64: combine the two scalars by
                                    allgathering the per-rank partials and
                                    summing them in rank order (as multi-shard
                                    mode always does) instead of ncclAllReduce:
                                    results independent of RCCL's algorithm and
                                    bitwise equal to the multi-shard run with the
                                    same partition */
#define CGX_SYMMETRIC    0x8000 /* fp64, one GPU: keep only the upper triangle of
                                   A, in 128 x 128 tiles, and compute A.p from
                                   it (half the bytes per matVec).  CG requires
                                   a symmetric A; this mode reads only
                                   A[i][j] for j >= 128*(i/128) (the lower
                                   triangle outside the diagonal tiles is never
                                   read).  With CGX_HOST_STREAM the tiles stay
                                   in pinned host memory and stream in chunks.
                                   Sums run in a different order than
                                   the row-major kernel: results agree to fp64
                                   rounding, deterministically. */
#define CGX_HOST_STREAM  0x200 /* keep A in pinned host memory and stream row
                                  tiles through the GPU every matVec (out-of-HBM
                                  systems; tile size CGX_STREAM_TILE_MB, default
                                  256, copy streams CGX_STREAM_COPIES, default 2) */
#define CGX_PHASES       0x10000 /* dense fp64 (row-major, resident A): the
                                    kernels of every iteration on the first
                                    shard stamp their start and end on the
                                    device's constant clock -- nothing is
                                    inserted between them -- and
                                    cgx_get_phase_times() turns the stamps into
                                    phase durations after the fact */
#define CGX_PEER_ACTIVE  0x20000 /* reported in cgx_info.flags: a multi-shard
                                    context spans distinct devices and peer
                                    access is enabled between every pair of
                                    them (the exchange kernels then read
                                    peers' memory over xGMI) */
#define CGX_SMALL_ACTIVE 0x40000 /* reported in cgx_info.flags: one GPU, one
                                    resident fp64 row block of 2048..8192
                                    columns -- the matVec stages the vector in
                                    LDS, one block per CU (k_matvec_small_f64;
                                    CGX_MV_SMALL=0 turns it off) */
#define CGX_FOLD_ACTIVE  0x80000 /* reported in cgx_info.flags: the two-launch
                                    iteration folds p = r + beta p into the
                                    next matVec (CGX_FOLD_P) */
#define CGX_XDEFER_ACTIVE 0x100000 /* reported in cgx_info.flags: the fused
                                    Poisson iteration updates x only every
                                    other or every third iteration (60 / 58.7
                                    instead of 64 B per grid point; x the same
                                    bits after every cgx_iterate call;
                                    CGX_POISSON_XDEFER=0: every iteration) */
#define CGX_XDEFER3_ACTIVE 0x200000 /* reported in cgx_info.flags with
                                    CGX_XDEFER_ACTIVE: every third iteration
                                    (the default, a third p slab;
                                    CGX_POISSON_XDEFER=2: every other) */
/* Reported in cgx_info.flags: how a context with several row blocks
 * exchanges, so a caller (bench.py) can say what ran. */
#define CGX_PULL_ACTIVE   0x400000 /* one process: the exchange runs as pull
                                    kernels on each consuming block's stream
                                    (else one hipMemcpyPeerAsync per block pair,
                                    CGX_LOCAL_XCHG=copy) */
#define CGX_FOLDED_ACTIVE 0x800000 /* one process, fp64: both scalar combines
                                    summed in rank order by the kernels that
                                    consume them (else a combine kernel per
                                    block and scalar, CGX_LOCAL_FUSE=0) */
#define CGX_HALO_PULL_ACTIVE 0x1000000 /* one process, fused Poisson: r's halo
                                    rows read in place from the neighbouring
                                    slabs by k_poisson_p (no halo copies) */
#define CGX_THREADS_ACTIVE 0x2000000 /* one process: one host thread per row
                                    block enqueues its work (CGX_LOCAL_THREADS=1) */
#define CGX_HALO_OVERLAP_ACTIVE 0x4000000 /* fused Poisson over slabs in rank
                                    mode (or copies): r's halo exchange runs on
                                    the comm stream beside k_poisson_p's
                                    interior (CGX_HALO_OVERLAP=0: before it) */

#define CGX_CSR_ACTIVE 0x8000000   /* reported in cgx_info.flags: a cgx_create_csr context */
#define CGX_PRECOND_ACTIVE 0x10000000 /* reported in cgx_info.flags: a cgx_create_csr context iterating
                                         with a diagonal preconditioner (cgx_set_precond) */
#define CGX_CSR_HALO_ACTIVE 0x20000000 /* reported in cgx_info.flags: a cgx_create_csr_multi context whose
                                         row blocks exchange p by index lists (k_gather_indexed; else whole
                                         slices: CGX_CSR_XCHG=full, CGX_LOCAL_XCHG=copy, or one block) */
#define CGX_BSR_ACTIVE 0x40000000 /* reported in cgx_info.flags: a cgx_create_csr context that is block-valued
                                     (cgx_set_bsr), beside CGX_CSR_ACTIVE */

typedef struct cgx_ctx cgx_ctx;

/* Opaque RCCL bootstrap id (ncclUniqueId is 128 bytes). */
typedef struct { char bytes[128]; } cgx_unique_id;

typedef struct {
    int64_t n;            /* global system size                               */
    int64_t lda;          /* device leading dimension (n rounded up to 128;
                             CGX_A_F32: to 256, in floats; cgx_create_csr:
                             the vectors' pitch)                               */
    int     nranks;       /* row blocks in the whole job                      */
    int     nshards;      /* row blocks driven by this process                */
    int     rank0;        /* global index of this process's first row block   */
    int64_t row0;         /* first global row owned by this process           */
    int64_t nrows;        /* rows owned by this process                       */
    int     flags;
    int     elem_bytes;   /* 8 (CGX_F64, CGX_A_F32) or 4 (CGX_F32_REF)        */
} cgx_info;

typedef struct {
    int64_t iterations;    /* loop iterations of the last solve (k+1 at break) */
    int     converged;     /* 1 if sqrt(r.r) < eps ended the loop              */
    double  rr;            /* last r.r (global)                                */
    double  solve_ms;      /* host wall time of the last cgx_solve             */
    double  matvec_ms;     /* sum of timed matVec kernel durations (CGX_TIMING)*/
    int64_t matvec_count;  /* matVec launches timed                            */
    int64_t total_iterations; /* iterations since the context was created     */
} cgx_stats;

/* Per-phase times of the iterations since the last cgx_reset_timing (or since
 * creation), CGX_PHASES contexts: for each phase the median and the mean over
 * the iterations, in microseconds, and the number of samples.  Phases follow
 * parallel_cg.c's loop (:288-323) on the first shard's stream: a kernel's own
 * span (first block's start to last block's end), or the span between two
 * consecutive kernels -- the exchange enqueued between them, or a launch gap.
 * Consecutive phases tile the iteration: MATVEC_OWN + GATHER_EXPOSED + MATVEC
 * + COMBINE_PAP + UPDATE_R + COMBINE_RR + UPDATE_XP + GAP = ITERATION. */
#define CGX_PH_MATVEC_OWN     0 /* overlap: own-column-block matVec (p local)   */
#define CGX_PH_GATHER_EXPOSED 1 /* the compute stream waiting for p's allgather
                                   (overlap: from the end of the own-block
                                   launch to the start of the rest launch,
                                   which waits for the allgather on the same
                                   stream; otherwise the whole allgather,
                                   launch gap included) parallel_cg.c:290-291 */
#define CGX_PH_MATVEC         2 /* the matVec with p.Ap (overlap: the rest
                                   launch, accumulating onto the own block's
                                   row sums, with p.Ap)               :292-293 */
#define CGX_PH_COMBINE_PAP    3 /* MPI_Allreduce(p.Ap) counterpart        :294   */
#define CGX_PH_UPDATE_R       4 /* r -= alpha Ap, r.r                     :304-309 */
#define CGX_PH_COMBINE_RR     5 /* MPI_Allreduce(r.r) counterpart         :313   */
#define CGX_PH_UPDATE_XP      6 /* x += alpha p, p = r + beta p  :299-303,318-322 */
#define CGX_PH_GAP            7 /* end of an iteration to the start of the next
                                   (host launch rate, lookahead waits)          */
#define CGX_PH_ITERATION      8 /* start of an iteration to the start of the next */
#define CGX_PH_MATVEC_BUSY    9 /* not a tile: the time the iteration's matVec
                                   kernels ran, the union of their spans (with
                                   the overlap: the own-block launch and the
                                   rest launch) -- the matVec's duration
                                   without the wait for p */
#define CGX_PH_COUNT         10
typedef struct {
    int64_t samples[CGX_PH_COUNT];
    double  median_us[CGX_PH_COUNT];
    double  mean_us[CGX_PH_COUNT];
} cgx_phase_times;

/* What the exchange runs on (rank mode): the communicator's rank count,
 * device and rank as RCCL reports them (ncclCommCount / ncclCommCuDevice /
 * ncclCommUserRank), and the PCI bus id of the context's device.  Other
 * modes: nranks = row blocks, rccl_device = -1. */
typedef struct {
    int  rccl_nranks;
    int  rccl_device;
    int  rccl_rank;
    int  device;
    char pci_bus_id[32];
} cgx_comm_info;

/* How the p exchange of an aligned multi-shard dense fp64 context was chosen
 * (parallel_cg.c:290-293: allgather p, then the matVec).  At creation the
 * context times both whole forms end to end on its own row blocks: overlap =
 * the real allgather (RCCL in rank mode, the pull kernels in one process) in
 * flight beside the own-column-block launch, then the rest launch; plain =
 * the allgather, then one launch over the whole row block.  The overlapped
 * form runs when overlap_form_us < (1 - margin) * plain_form_us.  In rank
 * mode every number is the max over ranks, so every rank decides alike.  The
 * parts are timed too and reported: the matVec split in two launches against
 * the one launch, and the allgather alone.  Times in microseconds, -1 when
 * not measured. */
#define CGX_OV_MEASURED 0 /* chosen from the measurement                     */
#define CGX_OV_FORCED   1 /* CGX_OVERLAP=1 / force: on                       */
#define CGX_OV_OFF      2 /* CGX_NO_OVERLAP or CGX_OVERLAP=0: off            */
#define CGX_OV_NA       3 /* no choice: one shard, unaligned blocks, fp32,
                             streamed A, p2p exchange                        */
typedef struct {
    int    active;         /* the overlapped form runs (CGX_OVERLAP_ACTIVE) */
    int    decided_by;     /* CGX_OV_*                                      */
    double allgather_us;   /* one allgather of p                            */
    double split_us;       /* own-block launch + rest launch                */
    double one_launch_us;  /* the one launch over the whole row block       */
    double split_cost_us;  /* split_us - one_launch_us (max over blocks)    */
    double overlap_form_us; /* the overlapped form, allgather included (the
                               slowest block, best of 2 passes of 2 forms
                               back to back)                                 */
    double plain_form_us;  /* the plain form: allgather, then one launch     */
    double margin;         /* the hysteresis of the decision (0.01)          */
    double forms_ms;       /* host wall time the end-to-end timing added to
                              the context's creation (this process)         */
} cgx_overlap_info;

/* ---- errors / info ------------------------------------------------------- */
const char *cgx_strerror(int code);
/* Detail message of the last failure on this thread ("" if none). */
const char *cgx_last_error(void);
int cgx_version(void);
int cgx_device_count(int *count);
/* The calling thread's pending HIP error (hipPeekAtLastError; 0 = none).
 * libcgx consumes the errors of the HIP calls it makes and reports them
 * through its own return codes, so this stays 0 across its entry points. */
int cgx_hip_last_error(void);
/* PCI bus id of a visible device ("0000:xx:yy.z"). */
int cgx_device_pci_bus_id(int device, char *buf, int len);
/* The link between two visible devices: *link_type as HSA reports it (4 =
 * xGMI, 2 = PCIe; -1 when HIP cannot tell), *hops, and *peer = 1 when
 * device_a can access device_b's memory directly (hipDeviceCanAccessPeer). */
int cgx_device_link(int device_a, int device_b, int *link_type, int *hops, int *peer);

/* ---- context lifetime ------------------------------------------------------ */
/* One GPU (device `device`).  Replaces serialConjugate.c's single process.
 * Dense n <= 16384 (no CGX_TIMING / CGX_PHASES / CGX_HOST_STREAM /
 * CGX_SYMMETRIC): the solve's kernels are launched once here, as no-ops, so
 * the first solve does not carry the runtime's first-launch cost
 * (CGX_WARM=0: not). */
int cgx_create(cgx_ctx **ctx, int64_t n, int device, int flags);

/* One process driving `nshards` row blocks on devices[0..nshards-1] (a device
 * may repeat: several row blocks on one GPU).  Exchange by pull kernels on
 * each consuming block's stream: one gather of p (k_gather_slices), one
 * rank-order combine per scalar (k_combine_peers); CGX_LOCAL_XCHG=copy:
 * one hipMemcpyPeerAsync per block pair instead (the same bits). */
int cgx_create_multi(cgx_ctx **ctx, int64_t n, int nshards, const int *devices, int flags);

/* One process per GPU (parallel_cg.c's one MPI rank per process): this
 * process owns row block `rank` of `nranks`; `id` comes from
 * cgx_get_unique_id() on rank 0 and is broadcast by the caller.  Exchange by
 * RCCL (allgather p, allreduce p.Ap and r.r) on the context's stream.
 * Fail-fast (the reference stops the job with MPI_Abort, parallel_cg.c:79-94):
 * the communicator's initialisation and every host wait are bounded by a
 * deadline of CGX_RCCL_TIMEOUT_S seconds (environment, default 60; 0 = wait
 * forever), and the waits watch RCCL's asynchronous error.  A rank that never joins,
 * dies, or issues a different collective makes the others' calls return
 * CGX_ERR_RCCL (naming the exchange and iteration) instead of hanging; the
 * communicator is then aborted and the context only accepts cgx_destroy. */
int cgx_get_unique_id(cgx_unique_id *id);
/* Loads RCCL (done on first rank-mode use anyway) and checks that every entry
 * point libcgx calls is present: CGX_OK, or CGX_ERR_RCCL with the reason in
 * cgx_last_error().  Needs no GPU.  A failed load is permanent for the process. */
int cgx_rccl_available(void);
int cgx_create_rank(cgx_ctx **ctx, int64_t n, int rank, int nranks,
                    const cgx_unique_id *id, int device, int flags);

/* Matrix-free 5-point 2D Poisson operator (configs[4]; no reference
 * counterpart): n = m*m unknowns on an m x m interior grid, Dirichlet zero
 * boundary, (A u)_ij = 4u_ij - u_(i-1)j - u_(i+1)j - u_i(j-1) - u_i(j+1),
 * natural row-major order.  Multi-GPU splits the grid into slabs of m/P grid
 * rows (m % P == 0) and exchanges one halo row with each neighbour per
 * iteration (ncclSend/Recv in rank mode) instead of allgathering p.
 * CGX_F64 only; set b / x0 with cgx_fill or cgx_set_rows (A must be NULL).
 * Pinned by tests/test_gpu_poisson_probe.py on rough (random, nonzero) b and
 * x0, one block to eight, fused and split, every x deferral, every halo
 * exchange form and two ranks: after a fixed count of iterations every element
 * of x agrees with sequential CG in extended precision to fp64 rounding (100 x
 * the spread between fp64 summation orders, at most 1.2e-11 of max|x|) under
 * every key of CGX_POISSON_PLAN; x and r.r are bit-identical across `rb` on a
 * given grid, and the same bits when a plan runs twice; `rows`, `bands`,
 * `reverse` and `blocks` change x only through the order in which the partial
 * sums of p.Ap and r.r are added (`pipe` not at all). */
int cgx_create_poisson(cgx_ctx **ctx, int64_t m, int device, int flags);
int cgx_create_poisson_multi(cgx_ctx **ctx, int64_t m, int nshards, const int *devices, int flags);
int cgx_create_poisson_rank(cgx_ctx **ctx, int64_t m, int rank, int nranks,
                            const cgx_unique_id *id, int device, int flags);

#define CGX_MAX_NRHS 8
/* One GPU, dense fp64, A resident row-major: nrhs (1..CGX_MAX_NRHS) systems
 * A x_j = b_j solved together, one read of A per iteration (see "Several
 * right-hand sides" above).  flags: CGX_F64, optionally with CGX_TIMING. */
int cgx_create_nrhs(cgx_ctx **ctx, int64_t n, int nrhs, int device, int flags);
int cgx_get_nrhs(const cgx_ctx *ctx, int *nrhs);          /* 1 for every other context */
/* Column j's iterations, converged and rr of the last solve (the other
 * fields as cgx_get_stats).  j = 0 on any other context: cgx_get_stats. */
int cgx_get_stats_rhs(cgx_ctx *ctx, int j, cgx_stats *st);
/* True residuals of the current x: rnorm[j] = ||b_j - A x_j||_2, bnorm[j] =
 * ||b_j||_2, nrhs entries each; either may be NULL.  Overwrites r and p: ends
 * a solve in progress.  (Any other context: one entry, cgx_residual_norm's.) */
int cgx_residual_norms(cgx_ctx *ctx, double *rnorm, double *bnorm);

/* ---- sparse A in CSR storage (see "Sparse A" above) ---------------------------- */
/* Host-only: CGX_OK, or CGX_ERR_SHAPE with the first offence named in cgx_last_error():
 * row_ptr[0] != 0, row_ptr decreasing at row i, row_ptr[n] != nnz, col_idx[e] outside [0, n). */
int cgx_csr_check(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col_idx);
/* One GPU, fp64, A as CSR with room for nnz entries.  flags: CGX_F64, optionally CGX_TIMING.
 * n < 2^31.  The arguments are checked before any device is touched. */
int cgx_create_csr(cgx_ctx **ctx, int64_t n, int64_t nnz, int device, int flags);
/* Host arrays (row_ptr[n] entries, at most the context's nnz); runs cgx_csr_check first and
 * uploads nothing when it fails (an earlier matrix stays as it was).  Ends a solve in progress. */
int cgx_set_csr(cgx_ctx *ctx, const int64_t *row_ptr, const int32_t *col_idx, const double *values);
/* cgx_set_csr with float values, which stay float on the device (see "Float-stored values"
 * above): the context gives the bits a double-valued one gives on (double)values[e].  The same
 * checks, refusals and effects as cgx_set_csr; a failed call also leaves the value type as it was. */
int cgx_set_csr_f32(cgx_ctx *ctx, const int64_t *row_ptr, const int32_t *col_idx, const float *values);
/* ---- block (BSR) storage on a cgx_create_csr context (see "Block storage" above) ---------- */
#define CGX_MAX_BSR_BLOCK 8
/* Host-only: cgx_csr_check's rules on a block structure of nb block rows and nb block columns:
 * brow_ptr[0] != 0, brow_ptr decreasing at block row I, brow_ptr[nb] != nnzb, bcol_idx[q] outside
 * [0, nb) -- CGX_ERR_SHAPE with the first offence named. */
int cgx_bsr_check(int64_t nb, int64_t nnzb, const int64_t *brow_ptr, const int32_t *bcol_idx);
/* Host arrays in scipy's bsr_matrix layout (brow_ptr[n / bs] blocks of bs x bs, nnzb * bs * bs at most
 * the context's nnz), 2 <= bs <= CGX_MAX_BSR_BLOCK; makes a plain cgx_create_csr context block-valued
 * until the next cgx_set_csr / cgx_set_csr_f32.  Checks and effects: "Block storage" above. */
int cgx_set_bsr(cgx_ctx *ctx, int bs, const int64_t *brow_ptr, const int32_t *bcol_idx, const double *values);
/* ---- diagonal (DIA) storage on a cgx_create_csr context (see "Diagonal storage" above) ---- */
/* Host-only: n >= 1, ndiag >= 0, every offset inside (-n, n) -- CGX_ERR_SHAPE names the first
 * offsets[k] outside and its value. */
int cgx_dia_check(int64_t n, int64_t ndiag, const int32_t *offsets);
/* Host arrays in scipy's dia_matrix layout (data[k * ld + j] = A[j - offsets[k]][j], ld >= n,
 * ndiag * n at most the context's nnz); makes a plain cgx_create_csr context diagonal-valued until
 * the next cgx_set_csr / cgx_set_csr_f32 / cgx_set_bsr.  Checks and effects: "Diagonal storage" above. */
int cgx_set_dia(cgx_ctx *ctx, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld);
/* ---- one-sided diagonal storage of a symmetric A (see "One-sided diagonal storage" above) ---- */
/* Host-only: n >= 1, ndiag >= 0, every offset inside [0, n) -- CGX_ERR_SHAPE names the first
 * offsets[k] outside and its value. */
int cgx_dia_sym_check(int64_t n, int64_t ndiag, const int32_t *offsets);
/* Host arrays in scipy's dia_matrix layout of triu(A) (data[k * ld + j] = A[j - offsets[k]][j] for j in
 * [offsets[k], n), ld >= n, ndiag * n at most the context's nnz); makes a plain cgx_create_csr context
 * one-sided until the next cgx_set_csr / cgx_set_csr_f32 / cgx_set_bsr / cgx_set_dia.  Symmetry cannot be
 * checked: only one triangle is given. */
int cgx_set_dia_sym(cgx_ctx *ctx, int64_t ndiag, const int32_t *offsets, const double *data, int64_t ld);
/* One GPU, fp64: nrhs (1..CGX_MAX_NRHS) systems A x_j = b_j on one CSR matrix with room for
 * nnz entries, solved together, one read of the CSR arrays per iteration.
 * flags: CGX_F64, optionally CGX_TIMING.  Arguments are checked before any device is touched. */
int cgx_create_csr_nrhs(cgx_ctx **ctx, int64_t n, int64_t nnz, int nrhs, int device, int flags);
/* One process, nshards row blocks of n / nshards rows on devices[0..nshards-1] (a device may
 * repeat), A as CSR, fp64.  nnz_block: room for that many entries in every row block.
 * flags: CGX_F64, optionally CGX_TIMING.  Arguments are checked before any device is touched. */
int cgx_create_csr_multi(cgx_ctx **ctx, int64_t n, int64_t nnz_block, int nshards,
                         const int *devices, int flags);
/* Host-only, no GPU: the exchange plan of a matrix over nshards equal row blocks.
 * counts[d * nshards + q] = how many distinct columns of block q's row range occur in block d's
 * rows (0 on the diagonal d == q).  The structure must pass cgx_csr_check (run first;
 * CGX_ERR_SHAPE as there); n % nshards != 0 is CGX_ERR_SHAPE. */
int cgx_csr_halo_counts(int64_t n, int nshards, const int64_t *row_ptr, const int32_t *col_idx,
                        int64_t *counts);
/* The list of one pair: counts[dst * nshards + src] offsets into block src (column - src's first
 * row), ascending, each once. */
int cgx_csr_halo_list(int64_t n, int nshards, const int64_t *row_ptr, const int32_t *col_idx,
                      int dst, int src, int32_t *offsets);
/* The counts in use on a live context (nshards * nshards entries); CGX_ERR_STATE before the first
 * cgx_set_csr, CGX_ERR_ARG on any other kind of context. */
int cgx_get_csr_halo(cgx_ctx *ctx, int64_t *counts);

/* ---- diagonal preconditioning of a cgx_create_csr context (see "Sparse A" above) ------------- */
#define CGX_PC_NONE   0
#define CGX_PC_JACOBI 1   /* M^-1 = 1 / diag(A), taken from the CSR arrays on the device */
#define CGX_PC_DIAG   2   /* M^-1 = a caller's positive vector (reported; set by cgx_set_precond_diag) */
/* Host-only: CGX_OK, or CGX_ERR_SHAPE naming the first entry that is not finite or not > 0
 * (CGX_ERR_ARG: n < 1 or minv NULL). */
int cgx_precond_diag_check(int64_t n, const double *minv);
int cgx_set_precond(cgx_ctx *ctx, int kind);            /* CGX_PC_NONE or CGX_PC_JACOBI */
int cgx_set_precond_diag(cgx_ctx *ctx, const double *minv);   /* n host values; runs the check first */
int cgx_get_precond(const cgx_ctx *ctx, int *kind);     /* CGX_PC_NONE on every other context */
int cgx_get_precond_diag(cgx_ctx *ctx, double *minv);   /* the n values in use; CGX_ERR_STATE when none or CGX_PC_BLOCK */

/* ---- block-Jacobi preconditioning of a cgx_create_csr context (see "Sparse A" above) --------- */
#define CGX_PC_BLOCK      3   /* M^-1 = the inverses of A's bs x bs diagonal blocks (reported by
                                 cgx_get_precond; set by cgx_set_precond_block[_values]) */
#define CGX_MAX_PC_BLOCK  8
/* Blocks: nblk = ceil(n / bs) of bs * bs doubles, block after block, row-major inside a block;
 * a short last block (n % bs rows) uses its leading entries, the rest is +0.0 on output and
 * ignored on input. */
/* Extracts the diagonal blocks on the device, inverts them on the host (cgx_precond_block_invert)
 * and uploads the inverses: a one-time cost.  2 <= bs <= CGX_MAX_PC_BLOCK.  CGX_ERR_SHAPE names the
 * lowest block that is not positive definite; the context then keeps the preconditioner it had. */
int cgx_set_precond_block(cgx_ctx *ctx, int bs);
/* The caller's inverse blocks (host); runs cgx_precond_block_check first and changes nothing when
 * it fails.  Their symmetry and definiteness are the caller's business. */
int cgx_set_precond_block_values(cgx_ctx *ctx, int bs, const double *W);
/* The block size and (W != NULL) the inverse blocks in use; CGX_ERR_STATE unless the kind is CGX_PC_BLOCK. */
int cgx_get_precond_block(cgx_ctx *ctx, int *bs, double *W);
/* Host-only, no GPU needed.  W_k = (L L^T)^-1 with D_k = L L^T, reading D_k's lower triangle only;
 * W_k is symmetric bit for bit.  CGX_ERR_SHAPE names the lowest block with a pivot that is not
 * finite or not > 0, its rows and the pivot (W is then unspecified). */
int cgx_precond_block_invert(int64_t n, int bs, const double *D, double *W);
/* Host-only: CGX_OK, or CGX_ERR_SHAPE naming the first used entry W[block][i][j] that is not
 * finite, or on the diagonal and not > 0 (CGX_ERR_ARG: n < 1, bs outside the range, W NULL). */
int cgx_precond_block_check(int64_t n, int bs, const double *W);
/* Kernel-level, device pointers as cgx_spmv_csr (row_ptr int64, col_idx int32, values double):
 * D (nblk * bs * bs doubles, the layout above) = A's diagonal blocks, each entry the sum from
 * +0.0 in stored order of the row's entries in that column.  The indices are not range-checked. */
int cgx_csr_diag_blocks(int64_t n, int bs, const void *row_ptr, const void *col_idx, const void *values, void *D,
                        void *stream);

int cgx_destroy(cgx_ctx *ctx);
int cgx_get_info(const cgx_ctx *ctx, cgx_info *info);
int cgx_get_comm_info(cgx_ctx *ctx, cgx_comm_info *info);
int cgx_get_overlap_info(const cgx_ctx *ctx, cgx_overlap_info *info);

/* ---- data in / out (host arrays; element type per flags: double, float with
 * CGX_F32_REF; with CGX_A_F32 A is float and b / x are double) ------------- */
/* Rows [row0, row0+nrows) of A (row-major, host leading dimension lda_host),
 * of b and of x0.  Any pointer may be NULL.  Rows this process does not own
 * are ignored, so every rank may pass the full system (MPI_Scatter /
 * MPI_Bcast, parallel_cg.c:111-115) or only its own block.  */
int cgx_set_rows(cgx_ctx *ctx, int64_t row0, int64_t nrows, const void *A_rows,
                 int64_t lda_host, const void *b_rows, const void *x_rows);
/* Whole system: A is n x n row-major, b and x0 have n entries. */
int cgx_set_system(cgx_ctx *ctx, const void *A, const void *b, const void *x0);
/* On-device synthetic SPD system (generateSPDmatrix.m style, counter hash):
 *   A_ij = 0.5*(u(i,j)+u(j,i)) + n*[i==j],  b_i = u_b(i),  x0 = 0,
 * u = splitmix64-finalised counter hash -> 53-bit uniform in [0,1). */
int cgx_generate_spd(cgx_ctx *ctx, uint64_t seed);
/* b = b_value and x0 = x_value everywhere (e.g. the Poisson config: b = 1, x0 = 0). */
int cgx_fill(cgx_ctx *ctx, double b_value, double x_value);
/* x (n entries, replicated result like parallel_cg.c's local_vectorX).
 * After a cgx_iterate that failed part-way (a HIP error, an RCCL deadline),
 * x may hold part of an iteration: cgx_get_x and cgx_residual_norm return
 * CGX_ERR_STATE until cgx_set_x defines x again or cgx_solve_begin starts a
 * new solve, and cgx_iterate refuses until cgx_solve_begin. */
int cgx_get_x(cgx_ctx *ctx, void *x);
int cgx_set_x(cgx_ctx *ctx, const void *x);

/* ---- the solve (conjugrad) -------------------------------------------------- */
/* x_inout may be NULL (use / leave the device-resident x).  eps < 0: never
 * stop early; max_iter < 0: n (the reference's `k < ROWS`).  Iterations past
 * exact convergence (p.Ap or the old r.r exactly 0, e.g. after r.r underflows
 * in a long fixed-count run) take alpha = beta = 0 in fp64, so x stays at the
 * solution; CGX_F32_REF divides as serialConjugate.c does (0/0 = NaN). */
int cgx_solve(cgx_ctx *ctx, void *x_inout, double eps, int64_t max_iter, cgx_stats *st);
/* serialConjugate.c's `conjugrad(A, b, x)` (:180-259) in one call, for a
 * literal function-level drop-in: `conjugrad(A, b, x);` becomes
 * `cgx_conjugrad(A, b, x, ROWS, CGX_F32_REF, 1.0e-6, -1, NULL);`.  Host
 * arrays as the reference passes them (A row-major n x n, b, x in / out;
 * float with CGX_F32_REF -- the reference's x bit for bit -- else double;
 * CGX_A_F32: the reference's float A beside double b and x),
 * one context on device 0 created, used and destroyed inside the call; st
 * may be NULL.  Repeated solves on one system: the context functions above. */
int cgx_conjugrad(const void *A, const void *b, void *x, int64_t n, int flags, double eps, int64_t max_iter,
                  cgx_stats *st);
/* The same solve in pieces: r0 = p0 = b - A x, then `count` iterations. */
int cgx_solve_begin(cgx_ctx *ctx);
int cgx_iterate(cgx_ctx *ctx, int64_t count, double eps, int64_t *done, int *converged);
int cgx_get_stats(cgx_ctx *ctx, cgx_stats *st);
/* CGX_PHASES: the per-phase times (resolves the recorded events; waits for
 * the work they mark). */
int cgx_get_phase_times(cgx_ctx *ctx, cgx_phase_times *out);
int cgx_reset_timing(cgx_ctx *ctx);
int cgx_synchronize(cgx_ctx *ctx);
/* The context's HIP stream of its first shard (hipStream_t as void*). */
void *cgx_stream(cgx_ctx *ctx);
/* Tuning of the fp64 matVec (k_matvec_f64): rows per wave (1,2,4,8), 128-column
 * chunks in flight per row (2,4,8), the A load policy (0 plain, 1 non-temporal
 * global loads, 2 software-pipelined default-policy loads, 8 software-
 * pipelined non-temporal = default; every R and U goes with each policy --
 * R=8 U=8 pipelined is accepted but spills to scratch, so the default plan
 * never picks it; all give the same row sums bit for bit,
 * test_matvec_f64_every_plan_bitwise_equal; the variants measured and not adopted are
 * in tools/microbench/matvec_variants.hip),
 * resident blocks per CU for the grid (<= 0: occupancy query).  Results do not
 * depend on the plan's R/U/policy; the p.Ap partial order depends on the grid
 * size.
 * CGX_A_F32 contexts (k_matvec_a32): exactly the instantiated plans -- (rows
 * per wave, 256-column chunks in flight) one of (1,4) (1,8) (2,4) (4,2) (4,4)
 * (8,2), load policy 2 (default-policy loads) or 8 (non-temporal), both
 * software-pipelined; anything else is CGX_ERR_ARG.  The same row sums bit
 * for bit under every one of them. */
int cgx_set_matvec_plan(cgx_ctx *ctx, int rows_per_wave, int chunks_in_flight, int nontemporal,
                        int blocks_per_cu);
int cgx_get_matvec_plan(cgx_ctx *ctx, int *rows_per_wave, int *chunks_in_flight, int *nontemporal,
                        int *blocks);
/* True residual of the current x: *rnorm = ||b - A x||_2, *bnorm = ||b||_2
 * (either may be NULL).  Overwrites r and p: ends a solve in progress. */
int cgx_residual_norm(cgx_ctx *ctx, double *rnorm, double *bnorm);

/* ---- kernel-level entry points (device pointers; unit parity) -------------- */
/* dtype: CGX_F64 or CGX_F32_REF (cgx_matvec also: CGX_A_F32).  stream:
 * hipStream_t or NULL.
 * The reducing calls (cgx_dot, cgx_residual, cgx_update_xr) share one
 * reduction workspace per device: issue them on one stream per device (or
 * order the streams), as the reference's single-threaded calls are ordered. */
int cgx_dev_malloc(void **ptr, size_t bytes);
int cgx_dev_free(void *ptr);
int cgx_memcpy_h2d(void *dst, const void *src, size_t bytes);
int cgx_memcpy_d2h(void *dst, const void *src, size_t bytes);
int cgx_dev_synchronize(void);
/* matVec: out[i] = sum_j A[i*lda + j] * v[j], i < rows, j < cols.
 * CGX_A_F32: A is float (lda in floats), v and out are double. */
int cgx_matvec(int dtype, const void *A, int64_t lda, int64_t rows, int64_t cols,
               const void *v, void *out, void *stream);
/* nrhs vectors per pass over A (fp64 only):
 * Out[j*ldo + i] = sum_c A[i*lda + c] * V[j*ldv + c], j < nrhs (1..CGX_MAX_NRHS).
 * Column j of Out is cgx_matvec(CGX_F64)'s result on column j of V bit for bit. */
int cgx_matvec_nrhs(const void *A, int64_t lda, int64_t rows, int64_t cols, int nrhs,
                    const void *V, int64_t ldv, void *Out, int64_t ldo, void *stream);
/* Kernel-level, device pointers, as cgx_matvec: out[i] = sum_e values[e] * v[col_idx[e]]
 * over e in [row_ptr[i], row_ptr[i+1]), i < rows; v has cols entries.
 * The indices must have passed cgx_csr_check: the kernel does not range-check them.
 * T comes from CGX_SPMV_PLAN="T=..,nt=..,bpc=.." (default T = 8). */
int cgx_spmv_csr(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx,
                 const void *values, const void *v, void *out, void *stream);
/* cgx_spmv_csr on float values (device pointer), widened exactly: the bits cgx_spmv_csr gives on
 * (double)values[e] at the same T.  Plan from CGX_SPMV_PLAN as above. */
int cgx_spmv_csr_f32(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx,
                     const float *values, const void *v, void *out, void *stream);
/* Kernel-level, device pointers: values_tiled (ceil(nnzb / 64) * 64 * bs * bs doubles) = values
 * (nnzb * bs * bs doubles, block after block, row-major inside a block) in k_bsr_mult_f64's tiled
 * layout, the pad of the last tile +0.0.  2 <= bs <= CGX_MAX_BSR_BLOCK. */
int cgx_bsr_tile_values(int64_t nnzb, int bs, const void *values, void *values_tiled, void *stream);
/* Kernel-level, device pointers: out[I*bs + i] = sum over the blocks q in [brow_ptr[I], brow_ptr[I+1])
 * and j < bs of B_q[i][j] * v[bcol_idx[q]*bs + j], I < nb, in the order of "Block storage" above; v has
 * ncolb * bs entries and is 16-byte aligned when bs is even (CGX_ERR_ARG otherwise), values_tiled comes
 * from cgx_bsr_tile_values.  The indices must have passed cgx_bsr_check: the kernel does not
 * range-check them.  T comes from CGX_BSMV_PLAN="T=..,nt=..,bpc=.." (default T = 8). */
int cgx_spmv_bsr(int64_t nb, int64_t ncolb, int bs, const void *brow_ptr, const void *bcol_idx,
                 const void *values_tiled, const void *v, void *out, void *stream);
/* Kernel-level, device pointers: out[i] = sum over k < ndiag with 0 <= i + offsets[k] < n of
 * data[k*ld + i + offsets[k]] * v[i + offsets[k]], i < n, in the order of "Diagonal storage" above;
 * offsets is int32[ndiag], data double[ndiag * ld], ld >= n.  An even ld with 16-byte aligned data
 * and v lets two rows per lane use 16-byte loads; the bits do not depend on it.  The offsets should
 * have passed cgx_dia_check; one outside (-n, n) adds no term.  The plan comes from
 * CGX_DIA_PLAN="R=..,U=..,nt=..,bpc=.." (default: the context's rule). */
int cgx_spmv_dia(int64_t n, int64_t ndiag, const void *offsets, const void *data, int64_t ld,
                 const void *v, void *out, void *stream);
/* Kernel-level, device pointers: out = A v, A the symmetric matrix whose upper diagonals offsets / data
 * hold, in the order of "One-sided diagonal storage" above -- bit for bit cgx_spmv_dia on the expansion;
 * offsets is int32[ndiag], data double[ndiag * ld], ld >= n.  The offsets should have passed
 * cgx_dia_sym_check; one outside [0, n) adds no term.  The plan comes from
 * CGX_DIA_SYM_PLAN="R=..,U=..,nt=..,bpc=.." (default: the context's rule). */
int cgx_spmv_dia_sym(int64_t n, int64_t ndiag, const void *offsets, const void *data, int64_t ld,
                     const void *v, void *out, void *stream);
/* Kernel-level, device pointers: Out[j*ldo + i] = sum_e values[e] * V[j*ldv + col_idx[e]],
 * j < nrhs.  Column j is cgx_spmv_csr's result on column j bit for bit at the same T.
 * The indices must have passed cgx_csr_check.  T comes from
 * CGX_SPMM_PLAN="T=..,nt=..,bpc=.." (default T = 8). */
int cgx_spmm_csr(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx,
                 const void *values, int nrhs, const void *V, int64_t ldv,
                 void *Out, int64_t ldo, void *stream);
/* cgx_spmm_csr on float values (device pointer), widened exactly: the bits cgx_spmm_csr gives on
 * (double)values[e] at the same T.  Plan from CGX_SPMM_PLAN as above. */
int cgx_spmm_csr_f32(int64_t rows, int64_t cols, const void *row_ptr, const void *col_idx,
                     const float *values, int nrhs, const void *V, int64_t ldv,
                     void *Out, int64_t ldo, void *stream);
/* Kernel-level, device pointers: dst[idx[e]] = src[idx[e]] for e < count (doubles; idx int32,
 * every value once, not range-checked).  The caller offsets dst. */
int cgx_gather_indexed(const void *src, const void *idx, int64_t count, void *dst, void *stream);
/* vecVec: *out_dev = a . b */
int cgx_dot(int dtype, int64_t n, const void *a, const void *b, void *out_dev, void *stream);
/* residual x2 + vecVec: r = b - Ax; p = b - Ax; *rr_dev = r.r (rr_dev may be NULL) */
int cgx_residual(int dtype, int64_t n, const void *b, const void *Ax, void *r, void *p,
                 void *rr_dev, void *stream);
/* alpha = *rsold_dev / *pAp_dev; x += alpha p; r -= alpha Ap; *rr_dev = r.r */
int cgx_update_xr(int dtype, int64_t n, void *x, void *r, const void *p, const void *Ap,
                  const void *rsold_dev, const void *pAp_dev, void *rr_dev, void *stream);
/* p = r + (*rr_dev / *rsold_dev) p */
int cgx_update_p(int dtype, int64_t n, void *p, const void *r, const void *rr_dev,
                 const void *rsold_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CGX_H */
