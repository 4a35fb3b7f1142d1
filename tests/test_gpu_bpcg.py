"""cgx_set_precond_block: block-Jacobi preconditioning of cgx_create_csr contexts (cgx_pcg_block.hip), through every
layer -- the extracted blocks' bits, the inverse, the refusals, solves against the CPU reference
(tests/_bpcg_ref.py, whose docstring holds the systems and the measured margins), the host forms, the lifecycle and
`cg_hip --csr --block-jacobi`.

The bar is the project's fp64 one: the reference's loop count (asserted where the reference alone stands a factor of
3 from the threshold on both sides, which every case of the table does), ||x - x_ref|| <= 1e-10 ||x_ref||,
||b - A x|| <= max(1e-10 ||b||, 1e-10)."""
import os
import subprocess

import numpy as np
import pytest

import _bpcg_ref as br
import _pcg_ref as pr
import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
EPS, TOL = br.EPS, br.TOL
ERR_ARG, ERR_SHAPE, ERR_STATE = -1, -4, -6
# None on a tree without the feature: every test then fails at its first use
set_block = getattr(cg.Solver, "set_precond_block", None)
diag_blocks = getattr(cg, "csr_diag_blocks", None)
block_invert = getattr(cg, "precond_block_invert", None)
PRECOND_ACTIVE = cg.CGX_PRECOND_ACTIVE


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert set_block is not None, "the package has no block preconditioner"


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def bits(v):
    return np.float64(v).view(np.uint64)


def csr_solver(csr, b, precond=None):
    s = cg.Solver.from_csr(*csr, precond=precond)
    s.set_rows(0, b_rows=b, x_rows=np.zeros(b.size))
    return s


def no_hip_error():
    assert cg.lib().cgx_hip_last_error() == 0


def code_of(call):
    with pytest.raises(cg.CgxError) as e:
        call()
    return e.value.code, str(e.value)


# ---- 1. the extracted blocks' bits -------------------------------------------------------------------------------------
def hand_made():
    """test_gpu_pcg.py's 6-row matrix: columns unsorted, row 2's diagonal stored three times."""
    rows = [([3, 0], [0.5, 4.0]), ([1, 5, 0], [3.0, -0.25, 0.5]), ([2, 4, 2, 0, 2], [0.1, 1.0, 0.2, -0.5, 0.3]),
            ([5, 3, 0], [0.125, 7.0, 0.5]), ([2, 4], [1.0, 2.5]), ([3, 1, 5], [0.125, -0.25, 1.5])]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    indices = np.concatenate([c for c, _ in rows]).astype(np.int32)
    data = np.concatenate([v for _, v in rows]).astype(np.float64)
    return indptr, indices, data


def blocks_in_stored_order(csr, bs):
    """The numpy restatement: every entry added to its slot from +0.0 in stored order."""
    indptr, indices, data = csr
    n = indptr.size - 1
    D = np.zeros((br.nblocks(n, bs), bs, bs))
    for i in range(n):
        for e in range(indptr[i], indptr[i + 1]):
            j = int(indices[e]) - (i // bs) * bs
            if 0 <= j < bs:
                D[i // bs, i % bs, j] = D[i // bs, i % bs, j] + data[e]
    return D


@pytest.mark.parametrize("bs", range(2, 9))
def test_extraction_bits(bs):
    csr6 = hand_made()
    want = blocks_in_stored_order(csr6, bs)
    assert want[2 // bs, 2 % bs, 2 % bs] == (0.0 + 0.1 + 0.2) + 0.3 != (0.0 + 0.3 + 0.2) + 0.1
    assert same_bits(diag_blocks(*csr6, bs), want)
    A = br.block_scale_system(*br.base_system("masked", 1001, 2), bs, 4)[0]
    assert same_bits(diag_blocks(*pr.to_csr(A), bs), br.diag_blocks(A, bs))  # one term per sum
    no_hip_error()


# ---- 2. the inverse ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", range(2, 9))
def test_inverse_is_the_host_inversion_of_the_extracted_blocks(bs):
    A, csr, b, W, xo, K = br.system("masked", 1001, 2, 4, bs)
    with csr_solver(csr, b) as s:
        assert s.precond == "none" and not s.info.flags & PRECOND_ACTIVE
        s.set_precond_block(bs)
        assert s.precond == "block" and s.info.flags & PRECOND_ACTIVE
        got_bs, got = s.precond_block
        assert got_bs == bs and got.shape == (br.nblocks(1001, bs), bs, bs)
        assert same_bits(got, block_invert(diag_blocks(*csr, bs), 1001))
        used = np.zeros((bs, bs), bool)
        t = 1001 % bs or bs  # 1001 % bs is 1, 2, 1, 1, 5, 0, 1 for bs = 2 .. 8: a short last block but at bs = 7
        used[:t, :t] = True  # its unused slots +0.0
        assert same_bits(np.where(used, 0.0, got[-1]), np.zeros((bs, bs)))
    with cg.Solver.from_csr(*csr, precond=("block", bs)) as s:
        assert s.precond == "block" and same_bits(s.precond_block[1], got)
    no_hip_error()


# ---- 3. refused blocks ---------------------------------------------------------------------------------------------------
def broken(kind):
    """The 5 x 5 Poisson matrix (n = 25) with the diagonal of rows 17 and 9 spoiled; 9 is in the block to name."""
    indptr, indices, data = (a.copy() for a in pr.to_csr(oracle.poisson_dense(5)))
    for row in (17, 9):
        e = indptr[row] + int(np.flatnonzero(indices[indptr[row]:indptr[row + 1]] == row)[0])
        if kind == "missing":
            indices, data = np.delete(indices, e), np.delete(data, e)
            indptr[row + 1:] -= 1
        else:
            data[e] = {"zero": 0.0, "negative": -4.0, "nan": np.nan}[kind]
    return indptr, indices, data


@pytest.mark.parametrize("kind", ["missing", "zero", "negative", "nan"])
def test_refused_blocks(kind):
    csr = broken(kind)
    good = br.inverse_blocks(oracle.poisson_dense(5), 3)
    with csr_solver(csr, np.ones(25)) as s:
        # "jacobi" is not among the states: the spoiled diagonal refuses Jacobi itself (test_gpu_pcg.py), so that
        # state is reached on another matrix, test_refused_blocks_from_jacobi below
        for state in ("none", "diag", "block"):
            if state == "diag":
                s.set_precond(np.full(25, 0.5))
            elif state == "block":
                s.set_precond_block(3, values=good)
            x_before, st_before = s.solve(x0=np.zeros(25), eps=-1.0, max_iter=3)
            for bs, name in ((2, "block 4 (rows 8..9)"), (4, "block 2 (rows 8..11)"), (8, "block 1 (rows 8..15)")):
                code, msg = code_of(lambda: s.set_precond_block(bs))
                assert code == ERR_SHAPE and name + ": pivot " in msg, msg
            assert s.precond == state
            if state == "diag":
                assert same_bits(s.precond_diag(), np.full(25, 0.5))
            if state == "block":
                assert s.precond_block[0] == 3 and same_bits(s.precond_block[1], good)
            x_after, st_after = s.solve(x0=np.zeros(25), eps=-1.0, max_iter=3)
            assert same_bits(x_after, x_before) and bits(st_after.rr) == bits(st_before.rr)
    no_hip_error()


def test_refused_blocks_from_jacobi():
    """The state the spoiled diagonal cannot reach through Jacobi: rows 17 and 9 keep a positive diagonal, and the
    blocks are indefinite through their off-diagonal entries (|a_89| = 9 > sqrt(a_88 a_99))."""
    A = oracle.poisson_dense(5).copy()
    A[8, 9] = A[9, 8] = 9.0
    A[16, 17] = A[17, 16] = 9.0
    with csr_solver(pr.to_csr(A), np.ones(25), precond="jacobi") as s:
        minv = s.precond_diag()
        x_before, st_before = s.solve(x0=np.zeros(25), eps=-1.0, max_iter=3)
        code, msg = code_of(lambda: s.set_precond_block(2))
        assert code == ERR_SHAPE and "block 4 (rows 8..9): pivot 1 " in msg, msg
        assert s.precond == "jacobi" and same_bits(s.precond_diag(), minv)
        x_after, st_after = s.solve(x0=np.zeros(25), eps=-1.0, max_iter=3)
        assert same_bits(x_after, x_before) and bits(st_after.rr) == bits(st_before.rr)
    no_hip_error()


# ---- 4. solves -----------------------------------------------------------------------------------------------------------
def meets_bar(x, st, A, b, xo, K):
    print(f"loops {st.iterations} (reference {K}), rel x {rel(x, xo):.3e}, "
          f"residual {np.linalg.norm(b - A @ x):.3e}, sqrt(rr) {np.sqrt(st.rr):.3e}")
    assert st.converged == 1 and st.iterations == K, (st.iterations, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), EPS)
    assert np.sqrt(st.rr) < EPS  # stats.rr is r.r, the quantity the loop stopped on


@pytest.mark.parametrize("case", list(br.TABLE), ids=str)
def test_solve(case):
    A, csr, b, W, xo, K = br.system(*case)
    bs = case[4]
    assert K == br.TABLE[case][0]
    with csr_solver(csr, b, precond=("block", bs)) as s:
        x, st = s.solve(eps=EPS)
        meets_bar(x, st, A, b, xo, K)
        rn, bn = s.residual_norm()  # the true residual, as on a plain context
        assert abs(rn - np.linalg.norm(b - A @ x)) <= 1e-12 * np.linalg.norm(b)
        s.set_precond_block(bs, values=W)  # the reference's own blocks handed in: the same solve
        assert s.precond == "block" and same_bits(s.precond_block[1], W)
        x, st = s.solve(x0=np.zeros(b.size), eps=EPS)
        meets_bar(x, st, A, b, xo, K)
    no_hip_error()


# ---- 5. diagonal blocks are the diagonal kind ----------------------------------------------------------------------------
def test_diagonal_blocks_are_the_diagonal_kind():
    """The header's order makes z the same bits as CGX_PC_DIAG's; the dots' order may differ, so x is compared to
    TOL and the loop count exactly (point Jacobi on this system stands far from the threshold: 18 loops, asserted
    against the reference's count where it keeps the factor of 3)."""
    A, csr, b, _, _, _ = br.system("masked", 1001, 2, 4, 3)
    minv = 1.0 / np.diag(A)
    W = np.zeros((br.nblocks(1001, 3), 3, 3))
    i = np.arange(1001)
    W[i // 3, i % 3, i % 3] = minv
    xr, Kr, _, _ = br.checked(A, b, br.diag_apply(minv), require=False)
    with csr_solver(csr, b, precond=minv) as s:
        assert s.precond == "diag"
        xd, std = s.solve(eps=EPS)
        s.set_precond_block(3, values=W)
        assert s.precond == "block"
        xb, stb = s.solve(x0=np.zeros(1001), eps=EPS)
    assert (stb.iterations, stb.converged) == (std.iterations, 1)
    assert Kr is None or stb.iterations == Kr
    assert rel(xb, xd) <= TOL
    no_hip_error()


# ---- 6. host forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 16])
@pytest.mark.parametrize("case", [("masked", 1001, 2, 4, 3), ("masked", 2101, 8, 2, 8)], ids=str)
def test_host_forms(monkeypatch, case, T):
    A, csr, b, W, xo, K = br.system(*case)
    n = b.size
    monkeypatch.delenv("CGX_GATED", raising=False)
    with csr_solver(csr, b, precond=("block", case[4])) as s:
        s.set_matvec_plan(64 // T, 1, 8)
        x1, st1 = s.solve(x0=np.zeros(n), eps=EPS)  # device-gated
        meets_bar(x1, st1, A, b, xo, K)
        x1b, st1b = s.solve(x0=np.zeros(n), eps=EPS)  # again: the same bits
        assert same_bits(x1b, x1) and (st1b.iterations, bits(st1b.rr)) == (K, bits(st1.rr))
        monkeypatch.setenv("CGX_GATED", "0")  # host-checked
        x2, st2 = s.solve(x0=np.zeros(n), eps=EPS)
        monkeypatch.delenv("CGX_GATED")
        assert same_bits(x2, x1) and (st2.iterations, st2.converged) == (K, 1) and bits(st2.rr) == bits(st1.rr)
        x3, st3 = s.solve(x0=np.zeros(n), eps=-1.0, max_iter=K)  # fixed count
        assert same_bits(x3, x1) and st3.iterations == K and bits(st3.rr) == bits(st1.rr)
        s.set_x(np.zeros(n))  # in pieces
        s.begin()
        assert s.iterate(1) == (1, False) and s.iterate(2) == (2, False)
        done, conv = s.iterate(100, eps=EPS)
        assert (3 + done, conv) == (K, True)
        assert same_bits(s.get_x(), x1) and s.stats().iterations == K and bits(s.stats().rr) == bits(st1.rr)
        assert s.iterate(10, eps=EPS) == (0, True)  # nothing after convergence
    no_hip_error()


# ---- 7. the feature matters ----------------------------------------------------------------------------------------------
def test_jacobi_is_not_there_after_the_block_loop_count():
    A, csr, b, W, xo, K = br.system("masked", 1001, 2, 4, 8)
    with csr_solver(csr, b, precond="jacobi") as s:
        x, st = s.solve(eps=EPS, max_iter=K)
        assert (st.iterations, st.converged) == (K, 0) and np.sqrt(st.rr) > 1e3 * EPS
    no_hip_error()


# ---- 8. lifecycle --------------------------------------------------------------------------------------------------------
def test_lifecycle():
    A, csr, b, W, xo, K = br.system("masked", 1000, 2, 4, 4)
    _, _, _, W3, _, _ = br.system("masked", 1000, 2, 4, 3)  # only its shape matters below
    L = cg.lib()
    with cg.Solver(1000, csr_nnz=int(csr[0][-1])) as s:
        for call in (lambda: s.set_precond_block(4), lambda: s.set_precond_block(4, values=W)):
            assert code_of(call)[0] == ERR_STATE  # no matrix yet
        assert s.precond == "none"
        s.set_csr(*csr)
        s.set_rows(0, b_rows=b, x_rows=np.zeros(1000))
        x_plain, st_plain = s.solve(eps=-1.0, max_iter=9)
        # none -> block -> jacobi -> block (another bs) -> none
        s.set_precond_block(4)
        xb, stb = s.solve(x0=np.zeros(1000), eps=EPS)
        meets_bar(xb, stb, A, b, xo, K)
        assert code_of(s.precond_diag)[0] == ERR_STATE  # the block kind has no vector of values
        # a second solve with a new b on the same context
        b2 = 0.5 * b[::-1].copy()
        s.set_rows(0, b_rows=b2, x_rows=np.zeros(1000))
        x2, st2 = s.solve(eps=EPS)
        assert st2.converged == 1 and np.linalg.norm(b2 - A @ x2) <= max(TOL * np.linalg.norm(b2), EPS)
        # refusals that change nothing
        w4 = s.precond_block[1]
        for bad in (1, 9, 0, -3):
            code, msg = code_of(lambda: s.set_precond_block(bad))
            assert code == ERR_ARG, (bad, msg)
            assert code_of(lambda: s.set_precond_block(bad, values=W))[0] == ERR_ARG
        assert "CGX_PC_JACOBI" in code_of(lambda: s.set_precond_block(1))[1]
        assert L.cgx_set_precond(s._h, cg.PC_BLOCK) == ERR_ARG  # its own entry points, as CGX_PC_DIAG
        assert L.cgx_set_precond_block_values(s._h, 4, None) == ERR_ARG
        assert L.cgx_get_precond_block(s._h, None, None) == ERR_ARG
        worse = W.copy()
        worse[17, 2, 1] = np.inf
        code, msg = code_of(lambda: s.set_precond_block(4, values=worse))
        assert code == ERR_SHAPE and "W[17][2][1]" in msg, msg
        for wrong in (W3, W.astype(np.float32), W.reshape(-1)):
            with pytest.raises(ValueError):
                s.set_precond_block(4, values=wrong)
        assert s.precond == "block" and s.precond_block[0] == 4 and same_bits(s.precond_block[1], w4)
        s.set_precond("jacobi")
        assert s.precond == "jacobi" and same_bits(s.precond_diag(), 1.0 / np.diag(A))
        code, msg = code_of(lambda: s.precond_block)
        assert code == ERR_STATE, msg
        s.set_precond_block(8)
        assert s.precond == "block" and s.precond_block[0] == 8 and s.info.flags & PRECOND_ACTIVE
        s.set_rows(0, b_rows=b, x_rows=np.zeros(1000))
        x8, st8 = s.solve(eps=EPS)
        assert st8.converged == 1 and np.linalg.norm(b - A @ x8) <= max(TOL * np.linalg.norm(b), EPS)
        # off again: the plain bits are back
        s.set_precond(None)
        assert s.precond == "none" and not s.info.flags & PRECOND_ACTIVE
        assert code_of(lambda: s.precond_block)[0] == ERR_STATE
        x_back, st_back = s.solve(x0=np.zeros(1000), eps=-1.0, max_iter=9)
        assert same_bits(x_back, x_plain) and bits(st_back.rr) == bits(st_plain.rr)
        # cgx_set_csr turns it off
        s.set_precond_block(4)
        assert s.info.flags & PRECOND_ACTIVE
        s.set_csr(*csr)
        assert s.precond == "none" and not s.info.flags & PRECOND_ACTIVE
        x_again, _ = s.solve(x0=np.zeros(1000), eps=-1.0, max_iter=9)
        assert same_bits(x_again, x_plain)
    no_hip_error()


def test_other_contexts_refuse():
    csr = pr.to_csr(oracle.poisson_dense(4))
    makers = (lambda: cg.Solver(256), lambda: cg.Solver(256, nrhs=2), lambda: cg.Solver(None, poisson_m=16),
              lambda: cg.Solver.from_csr(*csr, nrhs=2))
    for make in makers:
        with make() as s:
            W = np.tile(np.eye(2), (br.nblocks(s.n, 2), 1, 1))
            for call in (lambda: s.set_precond_block(2), lambda: s.set_precond_block(2, values=W)):
                assert code_of(call)[0] == ERR_ARG
            assert s.precond == "none"
            code = code_of(lambda: s.precond_block)[0]
            assert code == (ERR_STATE if getattr(s, "csr_nnz", None) is not None else ERR_ARG)
    no_hip_error()


# ---- 9. CLI --------------------------------------------------------------------------------------------------------------
ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")


def test_cli_block_jacobi(tmp_path):
    n = 130
    A, b = br.block_scale_system(*pr.masked_base(n, 5), 3, 3)
    for name, arr, dec in (("A.txt", A, 6), ("b.txt", b, 9), ("x0.txt", np.zeros(n), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    Aw = cg.read_text(paths[0], n * n, np.float64).reshape(n, n)  # the matrix as the file holds it
    bw = cg.read_text(paths[1], n, np.float64)
    xo, K, before, at = br.checked(Aw, bw, br.block_apply(br.inverse_blocks(Aw, 3)), require=False)
    r = subprocess.run([cg.CLI_PATH, "--csr", "--block-jacobi", "3", "--eps", "1e-10", "--print-x", "--stats", *paths],
                       capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"Computing cg of matrix size : {n * n}"
    assert lines[2].startswith("iterations: ") and " converged: 1 " in lines[2], lines[2]
    if K is not None:  # the reference keeps the factor of 3 on this file
        assert lines[2].startswith(f"iterations: {K} converged: 1"), (lines[2], K, before, at)
    assert lines[3] == f"nnz: {np.count_nonzero(Aw)}"
    assert lines[4] == "precond: block-jacobi 3"
    x = np.array([float(v) for v in lines[-n:]])
    assert len(lines) == 5 + n and rel(x, xo) <= TOL
    assert np.linalg.norm(bw - Aw @ x) <= max(TOL * np.linalg.norm(bw), EPS)
    # a block the library refuses: its message, exit status 1
    Az = A.copy()
    Az[7, 7] = 0.0
    oracle.write_text(paths[0], Az, 6)
    r = subprocess.run([cg.CLI_PATH, "--csr", "--block-jacobi", "3", *paths], capture_output=True, text=True,
                       timeout=300, env=ONE_GPU)
    assert r.returncode == 1 and "cgx_set_precond_block" in r.stderr and "block 2 (rows 6..8)" in r.stderr, \
        (r.returncode, r.stderr)
