"""Block-Jacobi preconditioning of CSR contexts, the parts that need no GPU: the constants, the host-only inversion
of the diagonal blocks (cgx_precond_block_invert) and check of a caller's blocks (cgx_precond_block_check), the NULL
refusals of the context entry points, `cg_hip --block-jacobi`'s option checks (which run before any device is
touched), and the CPU reference itself (tests/_bpcg_ref.py) against its own table and np.linalg.solve."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _bpcg_ref as br
import conjugate_gradient_amd as cg

ERR_ARG, ERR_SHAPE = -1, -4
TOL = br.TOL
# None on a tree without the feature: every test then fails at its first use
PC_BLOCK = getattr(cg, "PC_BLOCK", None)
MAX_PC_BLOCK = getattr(cg, "CGX_MAX_PC_BLOCK", None)


def L_():
    L = cg.lib()
    assert hasattr(L, "cgx_precond_block_invert"), "libcgx has no block preconditioner"
    return L


def invert(n, bs, D):
    """(rc, message, W) of cgx_precond_block_invert on blocks in the header's layout."""
    L = L_()
    D = np.ascontiguousarray(D, np.float64)
    W = np.full(D.shape, np.nan)
    rc = L.cgx_precond_block_invert(n, bs, D.ctypes.data, W.ctypes.data)
    return rc, L.cgx_last_error().decode(), W


def check(n, bs, W):
    L = L_()
    rc = L.cgx_precond_block_check(n, bs, None if W is None else np.ascontiguousarray(W, np.float64).ctypes.data)
    return rc, L.cgx_last_error().decode()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_constants_match_header():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgx.h")) as f:
        hdr = dict((m.group(1), int(m.group(2), 0)) for m in re.finditer(r"#define\s+(CGX_\w+)\s+(0x[0-9a-fA-F]+|\d+)", f.read()))
    assert hdr.get("CGX_PC_BLOCK") == 3 and hdr.get("CGX_MAX_PC_BLOCK") == 8
    assert PC_BLOCK == 3 and MAX_PC_BLOCK == 8
    assert cg.PRECOND_KINDS == {"none": 0, "jacobi": 1, "diag": 2}  # the block kind has a constant of its own


# ---- inversion -------------------------------------------------------------------------------------------------------
def hold_inverse(n, bs, D):
    """W against np.linalg.inv per block: max|W - inv| <= 1e-10 max|inv| (the project's TOL: the blocks have
    condition <= 2.3e4, so two fp64 inversions differ by ~1e-12; numpy's own Cholesky-based inverse, inv(L)^T inv(L)
    with L = np.linalg.cholesky, stays within 1.4e-15 max|inv| of np.linalg.inv on every block of the table's
    systems, measured on the CPU, and is asserted below 1e-11 here); W symmetric bit for bit; unused slots +0.0."""
    rc, msg, W = invert(n, bs, D)
    assert rc == 0, msg
    assert same_bits(W, W.transpose(0, 2, 1))
    for k in range(D.shape[0]):
        t = min(bs, n - k * bs)
        inv = np.linalg.inv(D[k, :t, :t])
        assert np.abs(W[k, :t, :t] - inv).max() <= TOL * np.abs(inv).max(), (k, np.abs(W[k, :t, :t] - inv).max())
        Li = np.linalg.inv(np.linalg.cholesky(D[k, :t, :t]))
        assert np.abs(Li.T @ Li - inv).max() <= 1e-11 * np.abs(inv).max()
        used = np.zeros((bs, bs), bool)
        used[:t, :t] = True
        assert same_bits(np.where(used, 0.0, W[k]), np.zeros((bs, bs))), (k, W[k])  # +0.0, not -0.0, not NaN
    return W


@pytest.mark.parametrize("case", [c for c in br.TABLE if c[1] != 2101 or c[4] in (3, 8)], ids=str)
def test_invert_table_blocks(built, case):
    kind, size, seed, dec, bs = case
    A, _ = br.block_scale_system(*br.base_system(kind, size, seed), bs, dec)
    assert max(np.linalg.cond(A[k * bs:(k + 1) * bs, k * bs:(k + 1) * bs]) for k in range(br.nblocks(len(A), bs))) <= 2.3e4
    hold_inverse(A.shape[0], bs, br.diag_blocks(A, bs))


def test_invert_hand_made_short_last_block(built):
    """n = 8, bs = 3: blocks of 3, 3 and 2 rows.  Only the lower triangle is read: garbage above the diagonal and
    in the short block's unused slots changes nothing."""
    B0 = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]])
    B1 = np.array([[1e-3, 2e-3, 0.0], [2e-3, 5.0, 1.0], [0.0, 1.0, 7.0]])
    B2 = np.array([[2.0, -1.0], [-1.0, 2.0]])
    D = np.zeros((3, 3, 3))
    D[0], D[1], D[2, :2, :2] = B0, B1, B2
    W = hold_inverse(8, 3, D)
    G = D.copy()
    G[:, 0, 1] = G[:, 0, 2] = G[:, 1, 2] = 99.0
    G[2, 2, :] = G[2, :, 2] = np.nan
    rc, msg, Wg = invert(8, 3, G)
    assert rc == 0, msg
    assert same_bits(Wg, W)
    assert np.abs(W[2, :2, :2] - np.array([[2.0, 1.0], [1.0, 2.0]]) / 3.0).max() <= 4e-16
    # n < bs: one short block
    rc, msg, W1 = invert(2, 8, np.pad(B2, ((0, 6), (0, 6)))[None])
    assert rc == 0 and same_bits(W1[0, :2, :2], W[2, :2, :2]) and not W1[0, 2:, :].any() and not W1[0, :, 2:].any()


@pytest.mark.parametrize("bad,shown", [(0.0, "= -0.25 "), (-4.0, "= -4.25 "), (np.nan, "= nan "), (np.inf, "= inf ")])
def test_invert_names_the_lowest_block(built, bad, shown):
    """n = 25, bs = 2: rows 17 (block 8) and 9 (block 4) spoiled; block 4 (rows 8..9) is named, with the pivot
    (the spoiled diagonal entry less the 0.25 the first column's elimination takes)."""
    D = np.tile(np.array([[4.0, -1.0], [-1.0, 4.0]]), (13, 1, 1))
    D[12, 1, :] = D[12, :, 1] = 0.0  # the short last block: row 24 alone
    D[8, 1, 1] = bad
    D[4, 1, 1] = bad
    rc, msg, _ = invert(25, 2, D)
    assert rc == ERR_SHAPE, (rc, msg)
    assert "block 4 (rows 8..9): pivot 1 " in msg and shown in msg, msg
    assert "block 8" not in msg
    # a spoiled first pivot, and one that the elimination turns negative (an indefinite block with a positive diagonal)
    D2 = np.tile(np.array([[1.0, 2.0], [2.0, 1.0]]), (3, 1, 1))
    rc, msg, _ = invert(6, 2, D2)
    assert rc == ERR_SHAPE and "block 0 (rows 0..1): pivot 1 = -3 " in msg, msg
    D2[0] = [[bad, 0.0], [0.0, 1.0]]
    rc, msg, _ = invert(6, 2, D2)
    assert rc == ERR_SHAPE and "block 0 (rows 0..1): pivot 0 " in msg, msg


def test_invert_and_check_refuse_bad_arguments(built):
    D = np.ones((1, 2, 2))
    L = L_()
    for n, bs in ((0, 2), (-3, 2), (4, 1), (4, 0), (4, 9), (4, -2)):
        assert invert(n, bs, D)[0] == ERR_ARG, (n, bs)
        assert check(n, bs, D)[0] == ERR_ARG, (n, bs)
    assert "CGX_PC_JACOBI" in invert(4, 1, D)[1]  # bs == 1 points to point Jacobi
    assert L.cgx_precond_block_invert(2, 2, None, D.ctypes.data) == ERR_ARG
    assert L.cgx_precond_block_invert(2, 2, D.ctypes.data, None) == ERR_ARG
    assert check(2, 2, None)[0] == ERR_ARG


# ---- cgx_precond_block_check ---------------------------------------------------------------------------------------
def test_check_accepts_and_ignores_unused_slots(built):
    W = np.tile(np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.5], [0.0, 0.5, 1.0]]), (3, 1, 1))
    assert check(9, 3, W)[0] == 0
    W[2, 2, :] = W[2, :, 2] = np.nan  # n = 8: the last block is 2 x 2, its third row and column are ignored
    assert check(8, 3, W)[0] == 0
    assert check(9, 3, W)[0] == ERR_SHAPE
    assert check(2, 8, np.pad(np.eye(2), ((0, 6), (0, 6)), constant_values=np.nan)[None])[0] == 0  # n < bs


@pytest.mark.parametrize("where,bad,shown", [((1, 0, 1), np.nan, "W[1][0][1] = nan"), ((1, 2, 0), np.inf, "W[1][2][0] = inf"),
                                              ((1, 1, 1), 0.0, "W[1][1][1] = 0"), ((1, 1, 1), -2.0, "W[1][1][1] = -2"),
                                              ((0, 2, 2), -0.0, "W[0][2][2] = -0")])
def test_check_names_the_first_offence(built, where, bad, shown):
    W = np.tile(np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.5], [0.0, 0.5, 1.0]]), (3, 1, 1))
    W[2, 0, 0] = -1.0  # a later offence: not the one named
    W[where] = bad
    rc, msg = check(9, 3, W)
    assert rc == ERR_SHAPE and shown in msg, msg


# ---- NULL contexts -----------------------------------------------------------------------------------------------------
def test_entry_points_refuse_a_null_context(built):
    L = L_()
    b = ctypes.c_int(7)
    buf = np.ones(8)
    assert L.cgx_set_precond_block(None, 2) == ERR_ARG
    assert L.cgx_set_precond_block_values(None, 2, buf.ctypes.data) == ERR_ARG
    assert L.cgx_get_precond_block(None, ctypes.byref(b), buf.ctypes.data) == ERR_ARG and b.value == 7
    assert np.array_equal(buf, np.ones(8))
    # the kernel-level extraction: bad arguments are refused before the device is touched
    assert L.cgx_csr_diag_blocks(4, 2, None, None, None, None, None) == ERR_ARG
    assert L.cgx_csr_diag_blocks(4, 9, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) == ERR_ARG


def test_python_mirror_checks_before_the_c_call(built):
    s = cg.Solver.__new__(cg.Solver)
    s.n, s.dtype, s.flags, s._h = 7, np.dtype(np.float64), cg.CGX_F64, None
    with pytest.raises(ValueError, match="integer"):
        s.set_precond_block(2.5)
    with pytest.raises(ValueError, match="float64"):
        s.set_precond_block(2, values=np.ones((4, 2, 2), np.float32))
    with pytest.raises(ValueError, match=r"\(4, 2, 2\) needed"):
        s.set_precond_block(2, values=np.ones((3, 2, 2)))
    with pytest.raises(ValueError, match=r"\(3, 3, 3\) needed"):
        s.set_precond_block(3, values=np.ones(27))
    for bad in ("ilu", 7):  # set_precond's refusals stay
        with pytest.raises((cg.CgxError, ValueError)):
            s.set_precond(bad)


# ---- CLI ---------------------------------------------------------------------------------------------------------------
CSR_REFUSES = (["--fp32-ref"], ["--a-fp32"], ["--symmetric"], ["--gpus", "2"], ["--p2p"], ["--nrhs", "2"])


@pytest.mark.parametrize("args", [["--block-jacobi", "3"], ["--csr", "--block-jacobi", "3", "--jacobi"],
                                  *(["--csr", "--block-jacobi", "3", *e] for e in CSR_REFUSES),
                                  ["--csr", "--block-jacobi", "3", "--spd", "64"],
                                  *(["--csr", "--block-jacobi", v] for v in ("1", "9", "0", "-2", "2.5", "x", ""))],
                         ids=lambda a: " ".join(a))
def test_cli_block_jacobi_option_checks(built, tmp_path, args):
    """Exit status 2 and one line naming the option, before a file is opened or a device touched: the files named
    here do not exist."""
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    r = subprocess.run([cg.CLI_PATH, *args, *paths], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and "--block-jacobi" in lines[0], r.stderr
    assert r.stdout == ""


def test_cli_block_jacobi_without_a_value(built):
    r = subprocess.run([cg.CLI_PATH, "--csr", "--block-jacobi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.strip().splitlines() == ["--block-jacobi must be an integer in [2, 8]"]


# ---- the reference against its own table ---------------------------------------------------------------------------
def near(got, want, rel):
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("case", list(br.TABLE), ids=str)
def test_reference_table(case):
    """The row holds: the block loop count and both margins (checked asserts the factor of 3), the printed ratios to
    their printed digits (6 %) where they are not rounding noise, x against np.linalg.solve to TOL, and point
    Jacobi's loop count on the same system -- never fewer loops than block Jacobi."""
    kind, size, seed, dec, bs = case
    loops, before_t, at_t, jacobi_t = br.TABLE[case]
    A, b = br.block_scale_system(*br.base_system(kind, size, seed), bs, dec)
    x, K, before, at = br.checked(A, b, br.block_apply(br.inverse_blocks(A, bs)))
    assert K == loops
    if at_t >= 1e-3:
        assert near(at, at_t, 0.06), (at, at_t)
    if before_t <= 1e5:
        assert near(before, before_t, 0.06), (before, before_t)
    xs = np.linalg.solve(A, b)
    assert np.linalg.norm(x - xs) <= TOL * np.linalg.norm(xs)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), br.EPS)
    Kj, conv, _ = br.jacobi_loops(A, b)
    assert conv == 1 and Kj == jacobi_t and Kj >= K


def test_reference_covers_the_kernel_paths():
    """The cases reach n < bs, n % bs in {0, 1, 2}, odd n and more than one 256-thread workgroup of blocks."""
    ns = {(c[1] if c[0] == "masked" else c[1] ** 2, c[4]) for c in br.TABLE}
    assert any(n < bs for n, bs in ns)
    assert {n % bs for n, bs in ns if n >= bs} >= {0, 1, 2}
    assert any(n % 2 for n, _ in ns) and any(br.nblocks(n, bs) > 256 for n, bs in ns)


def test_jacobi_is_not_there_after_the_block_loop_count():
    """What test_gpu_bpcg.py's 'the feature matters' rests on: on masked (1001, 2) dec 4 at bs 8, point Jacobi
    capped at the block loop count is far from converged (it needs 35 loops)."""
    case = ("masked", 1001, 2, 4, 8)
    A, b = br.block_scale_system(*br.base_system(*case[:3]), 8, 4)
    K, conv, rnorm = br.jacobi_loops(A, b, max_iter=br.TABLE[case][0])
    assert (K, conv) == (7, 0) and rnorm > 1e3 * br.EPS


def test_diagonal_blocks_are_the_diagonal_kind():
    """Blocks whose off-diagonal entries are 0 and whose diagonal is 1 / diag(A): the reference's loop count and x
    are point Jacobi's."""
    A, b = br.block_scale_system(*br.base_system("masked", 1001, 2), 3, 4)
    minv = 1.0 / np.diag(A)
    W = np.zeros((br.nblocks(1001, 3), 3, 3))
    i = np.arange(1001)
    W[i // 3, i % 3, i % 3] = minv
    xb, Kb, cb, _ = br.pcg(A, b, br.block_apply(W))
    xd, Kd, cd, _ = br.pcg(A, b, br.diag_apply(minv))
    assert (Kb, cb) == (Kd, cd) and np.linalg.norm(xb - xd) <= TOL * np.linalg.norm(xd)
