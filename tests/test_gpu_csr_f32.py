"""cgx_set_csr_f32: float-stored CSR values with fp64 arithmetic (k_csr_mult_f64 with VT = float,
k_csr_diag_minv, k_csr_diag_blocks) through every layer.

The contract is bit equality, so no test here has a tolerance: widening a float is exact and the summation order
does not change, so a float-valued launch or context gives what a double-valued one gives on (double)values[e].
The products are held against the CPU statement of the order (tests/_spmv_order.py) on the widened values; the
solves against a double-valued context -- existing code -- on the widened values."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _pcg_probe as pp
import _spmv_order as so
import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
EPS = 1e-10
A_F32 = cg.CGX_A_F32
LDV, LDO = so.STRUCT_COLS + 1, so.STRUCT_ROWS + 2  # odd and even pitches that are not the sizes


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    yield
    assert cg.lib().cgx_hip_last_error() == 0


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def run_spmv(indptr, indices, data32, v, rows, cols, spare=3):
    assert data32.dtype == np.float32
    dv = cg.DeviceArray.from_host(v)
    dout = cg.DeviceArray.from_host(np.full(rows + spare, np.nan))
    cg.spmv_csr(indptr, indices, data32, dv, dout, rows, cols, a_f32=True)
    out = dout.to_host()
    dv.free()
    dout.free()
    assert np.isnan(out[rows:]).all(), "the kernel stored past the last row"
    return out[:rows]


def run_spmm(indptr, indices, data32, V, rows, cols, nrhs, ldv, ldo):
    """Out as (8, ldo) after one call on an Out pre-filled with NaN."""
    assert data32.dtype == np.float32
    dV = cg.DeviceArray.from_host(V)
    dO = cg.DeviceArray.from_host(np.full(8 * ldo, np.nan))
    cg.spmm_csr(indptr, indices, data32, dV, dO, rows, cols, nrhs, ldv=ldv, ldo=ldo, a_f32=True)
    out = dO.to_host().reshape(8, ldo)
    dV.free()
    dO.free()
    assert np.isnan(out[:, rows:]).all(), "the kernel stored past the last row"
    assert np.isnan(out[nrhs:]).all(), "the kernel stored a column >= nrhs"
    return out[:nrhs, :rows]


# ---- 1. product bits against the stated order: the structure matrix --------------------------------------------
@functools.lru_cache(maxsize=None)
def struct32():
    """The structure matrix with its values rounded to float; 18 of its row starts are odd, which puts those rows'
    4-byte loads off the 8-byte grid."""
    indptr, indices, data, v = so.structure_matrix()
    assert np.count_nonzero(indptr % 2) == 18 and indptr[-1] % 2 == 0
    data32 = data.astype(np.float32)
    assert not np.array_equal(data32.astype(np.float64), data)  # the rounding changed the values
    return frozen(indptr, indices, data32, v)


@functools.lru_cache(maxsize=None)
def struct_vcols():
    """8 vectors of STRUCT_COLS values at pitch LDV, column 0 the structure matrix's own v."""
    V = np.random.default_rng(31).standard_normal((8, LDV))
    V[0, :so.STRUCT_COLS] = struct32()[3]
    return frozen(V)[0]


@functools.lru_cache(maxsize=None)
def struct_expected(T):
    """The order statement on the widened values, per column."""
    indptr, indices, data32, _ = struct32()
    wide = data32.astype(np.float64)
    return frozen(np.stack([so.spmv_csr(indptr, indices, wide, struct_vcols()[j, :so.STRUCT_COLS], T)
                            for j in range(8)]))[0]


@pytest.mark.parametrize("nt", so.POLICIES)
@pytest.mark.parametrize("T", so.TS)
def test_structure_matrix_bits(monkeypatch, T, nt):
    indptr, indices, data32, v = struct32()
    want = struct_expected(T)
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt={nt}")
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt={nt}")
    out = run_spmv(indptr, indices, data32, v, so.STRUCT_ROWS, so.STRUCT_COLS)
    assert same_bits(out, want[0]), (T, nt, np.flatnonzero(bits(out) != bits(want[0])))
    for nrhs in (3, 8):
        outs = run_spmm(indptr, indices, data32, struct_vcols().ravel(), so.STRUCT_ROWS, so.STRUCT_COLS, nrhs, LDV, LDO)
        for j in range(nrhs):
            assert same_bits(outs[j], want[j]), (T, nt, nrhs, j, np.flatnonzero(bits(outs[j]) != bits(want[j])))


@pytest.mark.parametrize("nt", so.POLICIES)
@pytest.mark.parametrize("T", so.TS)
def test_structure_matrix_odd_nnz(monkeypatch, T, nt):
    """The structure matrix has 1680 entries; with one more entry on its last row the arrays end at an odd count, on
    a 4-byte boundary that is no 8-byte one.  Only the last row's sum changes."""
    indptr, indices, data32, v = struct32()
    indptr = indptr.copy()
    indptr[-1] += 1
    indices = np.concatenate([indices, [so.STRUCT_COLS - 1]]).astype(np.int32)
    data32 = np.concatenate([data32, [np.float32(-1.0 / 3.0)]]).astype(np.float32)
    assert indptr[-1] % 2 == 1
    s = int(indptr[-2])
    want = struct_expected(T).copy()
    V = struct_vcols()
    for j in range(8):
        want[j, -1] = so.spmv_row(indices[s:], data32[s:].astype(np.float64), V[j, :so.STRUCT_COLS], T)
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt={nt}")
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt={nt}")
    out = run_spmv(indptr, indices, data32, v, so.STRUCT_ROWS, so.STRUCT_COLS)
    assert same_bits(out, want[0]), (T, nt, np.flatnonzero(bits(out) != bits(want[0])))
    outs = run_spmm(indptr, indices, data32, V.ravel(), so.STRUCT_ROWS, so.STRUCT_COLS, 3, LDV, LDO)
    assert same_bits(outs, want[:3]), (T, nt)


def test_default_plan_is_the_double_call_s(monkeypatch):
    indptr, indices, data32, v = struct32()
    monkeypatch.delenv("CGX_SPMV_PLAN", raising=False)
    monkeypatch.delenv("CGX_SPMM_PLAN", raising=False)
    assert same_bits(run_spmv(indptr, indices, data32, v, so.STRUCT_ROWS, so.STRUCT_COLS), struct_expected(8)[0])
    outs = run_spmm(indptr, indices, data32, struct_vcols().ravel(), so.STRUCT_ROWS, so.STRUCT_COLS, 3, LDV, LDO)
    assert same_bits(outs, struct_expected(8)[:3])


# ---- 2. values that only a float path can get wrong -------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
ALL24 = 16777215.0 / 16777216.0  # 1 - 2^-24: all 24 significand bits set
TINY = (2.0 ** -149, 2.0 ** -127, -(2.0 ** -149), 2.0 ** -126, -0.0, 3 * 2.0 ** -149)  # denormals, FLT_MIN, -0.0
# per row: the values its entries cycle through.  The magnitudes are kept apart row by row, so that no row's sum
# rounds a wrong term away: beside FLT_MAX a flushed denormal would vanish in the rounding.
ROW_POOLS = ((FLT_MAX, -FLT_MAX, FLT_MAX * ALL24, 2.0 ** 127),  # 9 entries: the top of the range
             (-0.0,),                                           # 1 entry: -0.0 * v, and the sum from +0.0 is +0.0
             TINY,                                              # 70 entries: the bottom (they wrap at T = 64)
             (ALL24, 1.0 + 2.0 ** -23, -ALL24, 1.0 / 3.0, -0.0))  # 5 entries: full significands
ROW_LENS = (9, 1, 70, 5)


@functools.lru_cache(maxsize=None)
def special_matrix():
    """4 rows over 16 columns; v is of order 1 with full significands and mixed signs, so a product computed in
    float, or a value flushed to zero, changes bits of its row's sum."""
    indptr = np.concatenate([[0], np.cumsum(ROW_LENS)]).astype(np.int64)
    data = np.concatenate([[pool[k % len(pool)] for k in range(n)] for pool, n in zip(ROW_POOLS, ROW_LENS)])
    data32 = data.astype(np.float32)
    assert np.isfinite(data32).all()
    rng = np.random.default_rng(5)
    indices = rng.integers(0, 16, data32.size).astype(np.int32)
    v = rng.standard_normal(16)
    return frozen(indptr, indices, data32, v)


@pytest.mark.parametrize("nt", so.POLICIES)
@pytest.mark.parametrize("T", [2, 64])
def test_special_values(monkeypatch, T, nt):
    indptr, indices, data32, v = special_matrix()
    wide = data32.astype(np.float64)
    want = so.spmv_csr(indptr, indices, wide, v, T)
    assert np.isfinite(want).all() and abs(want[0]) > 1e37 and same_bits(want[1], 0.0) and 0 < abs(want[2]) < 1e-36
    # the reference itself tells the failures apart: denormals flushed to zero, or products rounded to float
    flushed = np.where(np.abs(wide) < 2.0 ** -126, 0.0, wide)
    assert not same_bits(so.spmv_csr(indptr, indices, flushed, v, T)[2], want[2])
    e = slice(int(indptr[3]), int(indptr[4]))
    prod32 = np.sum((data32[e] * v[indices[e]].astype(np.float32)).astype(np.float64))
    assert abs(prod32 - want[3]) > 1e-9 * abs(want[3])
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt={nt}")
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt={nt}")
    out = run_spmv(indptr, indices, data32, v, 4, 16)
    assert same_bits(out, want), (out, want)
    V = np.stack([v, -v, 0.5 * v])
    outs = run_spmm(indptr, indices, data32, V.ravel(), 4, 16, 3, 16, 4)
    for j in range(3):
        assert same_bits(outs[j], so.spmv_csr(indptr, indices, data32.astype(np.float64), V[j], T)), j


def test_denormals_alone(monkeypatch):
    """A row of float denormals only, times powers of two: each product is exact in fp64 and far from zero there."""
    data32 = np.array([2.0 ** -149, 2.0 ** -127, -(2.0 ** -149), 3 * 2.0 ** -149, 2.0 ** -130], np.float32)
    indptr, indices = np.array([0, 5], np.int64), np.arange(5, dtype=np.int32)
    v = np.array([2.0 ** 149, 2.0 ** 127, 2.0 ** 148, 2.0 ** 149, 2.0 ** 131])
    monkeypatch.setenv("CGX_SPMV_PLAN", "T=8,nt=2")
    assert same_bits(run_spmv(indptr, indices, data32, v, 1, 5), [1.0 + 1.0 - 0.5 + 3.0 + 2.0])


# ---- 3. the grid-stride walk, and one row -------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 8, 64])
def test_grid_stride_walk(monkeypatch, T):
    """70,000 rows under one block per CU: a wave walks several row groups and the last group is partial.  The
    tridiagonal values are signed powers of two, so they are floats already."""
    n = 70000
    indptr, indices, data = so.tridiag(n)
    data32 = data.astype(np.float32)
    assert np.array_equal(data32.astype(np.float64), data)
    rng = np.random.default_rng(7)
    v = rng.standard_normal(n)
    want = so.spmv_tridiag(n, v, T)
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt=8,bpc=1")
    out = run_spmv(indptr, indices, data32, v, n, n)
    assert same_bits(out, want), np.flatnonzero(bits(out) != bits(want))[:8]
    V = np.stack([v, rng.standard_normal(n), rng.standard_normal(n)])
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt=8,bpc=1")
    outs = run_spmm(indptr, indices, data32, V.ravel(), n, n, 3, n, n)
    for j in range(3):
        want = so.spmv_tridiag(n, V[j], T)
        assert same_bits(outs[j], want), (j, np.flatnonzero(bits(outs[j]) != bits(want))[:8])


@pytest.mark.parametrize("T", so.TS)
def test_one_row(monkeypatch, T):
    """n = 1 with 0, 1 and T + 1 entries (every column is 0: T + 1 duplicates are T + 1 terms)."""
    monkeypatch.setenv("CGX_SPMV_PLAN", f"T={T},nt=2")
    monkeypatch.setenv("CGX_SPMM_PLAN", f"T={T},nt=2")
    rng = np.random.default_rng(T)
    v = np.array([-1.2345678901234567])
    for length in (0, 1, T + 1):
        indptr = np.array([0, length], np.int64)
        indices = np.zeros(length, np.int32)
        data32 = rng.standard_normal(length).astype(np.float32)
        want = so.spmv_csr(indptr, indices, data32.astype(np.float64), v, T)
        assert same_bits(run_spmv(indptr, indices, data32, v, 1, 1), want), length
        outs = run_spmm(indptr, indices, data32, np.array([v[0], 0.75]), 1, 1, 2, 1, 1)
        assert same_bits(outs[0], want), length
        assert same_bits(outs[1], so.spmv_csr(indptr, indices, data32.astype(np.float64), np.array([0.75]), T)), length


# ---- 4. solve bits against the double-valued context -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def banded(n):
    """_pcg_probe's banded SPD system with its values rounded to float: (indptr, indices, data32, the widened
    values, b, x0).  The rounded matrix is still symmetric and strictly diagonally dominant (checked here, on the
    CPU), so it is SPD."""
    sy = pp.system(n)
    indptr, indices, data = sy.csr()
    data32 = data.astype(np.float32)
    wide = data32.astype(np.float64)
    assert not np.array_equal(wide, data)
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(indptr)), indices] = wide
    assert np.array_equal(A, A.T)
    d = np.diag(A)
    assert np.all(d > np.sum(np.abs(A), axis=1) - d)
    return frozen(indptr, indices, data32, wide, sy.b.copy(), sy.x0.copy())


def positive_array(n):
    return 0.1 + np.random.default_rng([n, 9]).random(n)


PRECONDS = ("none", "jacobi", "array", "block3", "block8")


def apply_precond(s, name, n):
    if name == "array":
        s.set_precond(positive_array(n))
    elif name.startswith("block"):
        s.set_precond(("block", int(name[5:])))
    elif name == "jacobi":
        s.set_precond("jacobi")


def pair(n, T=None):
    """(F, D): a float-valued context and a double-valued one on the widened values, b set."""
    indptr, indices, data32, wide, b, x0 = banded(n)
    F = cg.Solver.from_csr(indptr, indices, data32, a_f32=True)
    D = cg.Solver.from_csr(indptr, indices, wide)
    assert F.info.flags & A_F32 and not D.info.flags & A_F32
    assert F.info.elem_bytes == 8 and F.info.flags & cg.CGX_CSR_ACTIVE
    for s in (F, D):
        s.set_rows(0, b_rows=b, x_rows=x0)
        if T is not None:
            s.set_matvec_plan(64 // T, 1, 2)
    if T is not None:
        assert F.matvec_plan() == D.matvec_plan()  # the same grid: the fused p.Ap adds in the same order
    return F, D


def three_iterations(s, x0):
    s.set_x(x0)
    s.begin()
    assert s.iterate(3, eps=-1.0) == (3, False)
    return s.get_x()


def same_preconditioner(F, D, name):
    assert F.precond == D.precond
    if name in ("jacobi", "array"):
        assert same_bits(F.precond_diag(), D.precond_diag())
    if name.startswith("block"):
        (bf, Wf), (bd, Wd) = F.precond_block, D.precond_block
        assert bf == bd == int(name[5:]) and same_bits(Wf, Wd)


@pytest.mark.parametrize("T", [2, 16])
@pytest.mark.parametrize("name", PRECONDS)
@pytest.mark.parametrize("n", [257, 2049])
def test_solve_bits(monkeypatch, n, name, T):
    monkeypatch.delenv("CGX_GATED", raising=False)
    x0 = banded(n)[5]
    F, D = pair(n, T)
    with F, D:
        for s in (F, D):
            apply_precond(s, name, n)
        same_preconditioner(F, D, name)
        xf, xd = three_iterations(F, x0), three_iterations(D, x0)
        assert np.isfinite(xd).all() and not same_bits(xd, x0)
        assert same_bits(xf, xd), np.flatnonzero(bits(xf) != bits(xd))[:8]
        (xf, sf), (xd, sd) = F.solve(x0=x0, eps=EPS), D.solve(x0=x0, eps=EPS)
        assert sd.converged == 1 and sd.iterations > 3
        assert (sf.iterations, sf.converged) == (sd.iterations, sd.converged)
        assert same_bits([sf.rr], [sd.rr]) and same_bits(xf, xd)
        assert same_bits(F.residual_norm(), D.residual_norm())
        assert F.info.flags & A_F32 and bool(F.info.flags & cg.CGX_PRECOND_ACTIVE) == (name != "none")


def test_default_plan_solve_bits():
    """Without a chosen plan: both contexts take plan_spmv_csr's default T for the matrix."""
    x0 = banded(2049)[5]
    F, D = pair(2049)
    with F, D:
        assert F.matvec_plan() == D.matvec_plan()
        (xf, sf), (xd, sd) = F.solve(x0=x0, eps=EPS), D.solve(x0=x0, eps=EPS)
        assert sf.iterations == sd.iterations and same_bits([sf.rr], [sd.rr]) and same_bits(xf, xd)


@pytest.mark.parametrize("name", ["none", "block3"])
def test_host_checked_form(monkeypatch, name):
    n = 2049
    x0 = banded(n)[5]
    F, D = pair(n, 16)
    with F, D:
        for s in (F, D):
            apply_precond(s, name, n)
        monkeypatch.delenv("CGX_GATED", raising=False)
        xd, sd = D.solve(x0=x0, eps=EPS)
        monkeypatch.setenv("CGX_GATED", "0")
        xf, sf = F.solve(x0=x0, eps=EPS)
        assert (sf.iterations, sf.converged) == (sd.iterations, 1)
        assert same_bits([sf.rr], [sd.rr]) and same_bits(xf, xd)


@pytest.mark.parametrize("name", ["none", "jacobi"])
def test_iterate_in_pieces(monkeypatch, name):
    monkeypatch.delenv("CGX_GATED", raising=False)
    n = 257
    x0 = banded(n)[5]
    F, D = pair(n, 2)
    with F, D:
        for s in (F, D):
            apply_precond(s, name, n)
        xd, sd = D.solve(x0=x0, eps=EPS)
        F.set_x(x0)
        F.begin()
        assert F.iterate(2) == (2, False)
        assert F.iterate(1) == (1, False)
        done, conv = F.iterate(1000, eps=EPS)
        assert (3 + done, conv) == (sd.iterations, True)
        assert same_bits(F.get_x(), xd) and same_bits([F.stats().rr], [sd.rr])


# ---- 5. several right-hand sides ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 8])
@pytest.mark.parametrize("nrhs", [3, 8])
def test_nrhs_bits(monkeypatch, nrhs, T):
    monkeypatch.delenv("CGX_GATED", raising=False)
    n = 257
    indptr, indices, data32, wide, b, _ = banded(n)
    B = np.random.default_rng([n, nrhs]).random((nrhs, n)) - 0.5
    B[0] = b
    B[1] *= 1e-7  # a column that stops early and stays frozen while the others go on
    Z = np.zeros((nrhs, n))
    F = cg.Solver.from_csr(indptr, indices, data32, nrhs=nrhs, a_f32=True)
    D = cg.Solver.from_csr(indptr, indices, wide, nrhs=nrhs)
    with F, D:
        assert F.info.flags & A_F32 and not D.info.flags & A_F32
        res = []
        for s in (F, D):
            s.set_matvec_plan(64 // T, 1, 2)
            s.set_rows(0, b_rows=B, x_rows=Z)
            X, st = s.solve(eps=EPS)
            res.append((X, st, [s.stats_rhs(j) for j in range(nrhs)], s.residual_norms()))
        assert F.matvec_plan() == D.matvec_plan()
        (Xf, stf, rf, nf), (Xd, std, rd, nd) = res
        assert std.converged == 1 and (stf.iterations, stf.converged) == (std.iterations, 1)
        its = [r.iterations for r in rd]
        assert 0 < its[1] < min(its[:1] + its[2:]), its  # the scaled column froze first
        for j in range(nrhs):
            assert same_bits(Xf[j], Xd[j]), j
            assert (rf[j].iterations, rf[j].converged) == (rd[j].iterations, rd[j].converged), j
            assert same_bits([rf[j].rr], [rd[j].rr]), j
        assert same_bits(nf[0], nd[0]) and same_bits(nf[1], nd[1])


# ---- 6. switching the value type on one context -------------------------------------------------------------------------
def solve_record(s, x0):
    x, st = s.solve(x0=x0, eps=EPS)
    return bits(x).tolist(), st.iterations, bits([st.rr]).tolist()


def test_switching():
    n = 257
    indptr, indices, data32, wide, b, x0 = banded(n)
    thirds = wide / 3.0  # not floats: a stale float mode, or the floats left in the buffer's first half, would show
    assert not np.array_equal(thirds.astype(np.float32).astype(np.float64), thirds)
    L = cg.lib()
    with cg.Solver.from_csr(indptr, indices, wide) as D, cg.Solver.from_csr(indptr, indices, thirds) as D3:
        for s in (D, D3):
            s.set_rows(0, b_rows=b, x_rows=x0)
        want_f, want_3 = solve_record(D, x0), solve_record(D3, x0)
        D.set_precond("jacobi")
        want_fj = solve_record(D, x0)
    assert want_f != want_3 and want_f != want_fj
    with cg.Solver(n, csr_nnz=int(indptr[-1]) + 5) as s:
        s.set_rows(0, b_rows=b, x_rows=x0)
        s.set_csr(indptr, indices, data32, a_f32=True)
        assert s.info.flags & A_F32 and s.precond == "none"
        assert solve_record(s, x0) == want_f
        s.set_precond("jacobi")
        assert solve_record(s, x0) == want_fj
        s.set_csr(indptr, indices, thirds)  # double-valued again, and the preconditioner is off again
        assert not s.info.flags & A_F32 and s.precond == "none" and not s.info.flags & cg.CGX_PRECOND_ACTIVE
        assert solve_record(s, x0) == want_3
        s.set_precond(("block", 3))
        s.set_csr(indptr, indices, data32, a_f32=True)
        assert s.info.flags & A_F32 and s.precond == "none"
        assert solve_record(s, x0) == want_f
        s.set_precond("jacobi")
        # refused calls change nothing: the matrix, its value type and its preconditioner stay
        rp_bad = indptr.copy()
        rp_bad[7] = rp_bad[6] - 1
        ci_bad = indices.copy()
        ci_bad[11] = n
        rp_long = indptr.copy()
        rp_long[-1] += 6  # one entry more than the context has room for
        other = np.full(int(rp_long[-1]), 7.0, np.float32)
        ci_long = np.zeros(other.size, np.int32)
        for rp, ci, named in ((rp_bad, indices, "row_ptr"), (indptr, ci_bad, "col_idx"), (rp_long, ci_long, "room for")):
            rc = L.cgx_set_csr_f32(s._h, rp.ctypes.data, ci.ctypes.data, other.ctypes.data)
            assert rc == -4 and named in L.cgx_last_error().decode(), (rc, L.cgx_last_error())
            assert s.info.flags & A_F32 and s.precond == "jacobi"
        assert L.cgx_set_csr_f32(s._h, indptr.ctypes.data, None, None) == -1  # NULL arrays with nnz > 0
        assert solve_record(s, x0) == want_fj
        # ... and on a double-valued context a refused float call leaves it double-valued
        s.set_csr(indptr, indices, thirds)
        assert L.cgx_set_csr_f32(s._h, rp_bad.ctypes.data, indices.ctypes.data, other.ctypes.data) == -4
        assert not s.info.flags & A_F32
        assert solve_record(s, x0) == want_3
    with cg.Solver(n) as dense:  # not a CSR context
        assert L.cgx_set_csr_f32(dense._h, indptr.ctypes.data, indices.ctypes.data, data32.ctypes.data) == -1
        assert "cgx_set_csr_f32" in L.cgx_last_error().decode()
    assert L.cgx_hip_last_error() == 0


# ---- 7. CLI ---------------------------------------------------------------------------------------------------------------
ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")


def cli(*args):
    r = subprocess.run([cg.CLI_PATH, *args], capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


@pytest.mark.parametrize("pc", [[], ["--jacobi"], ["--block-jacobi", "3"]], ids=["plain", "jacobi", "block3"])
def test_cli_csr_a32(tmp_path, pc):
    """A banded matrix whose entries are multiples of 1/8, written with 4 decimals: every value of the file is a
    float, so `--csr-a32` and `--csr` hold the same matrix and print the same x."""
    m = 96
    rng = np.random.default_rng(96)
    A = np.diag(4.0 + rng.integers(0, 8, m) / 8.0)
    for d in (1, 2, 37):
        off = rng.integers(-4, 5, m - d) / 8.0
        A += np.diag(off, d) + np.diag(off, -d)
    b = rng.integers(-40, 41, m) / 8.0
    for name, arr, dec in (("A.txt", A, 4), ("b.txt", b, 4), ("x0.txt", np.zeros(m), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    Aw = cg.read_text(paths[0], m * m, np.float64)
    assert np.array_equal(Aw.astype(np.float32).astype(np.float64), Aw) and np.array_equal(Aw.reshape(m, m), A)
    common = ["--eps", "1e-10", "--print-x", "--stats", *pc, *paths]
    f32 = cli("--csr-a32", *common)
    f64 = cli("--csr", *common)
    assert "values: float" in f32 and "values: float" not in f64
    assert f32[2].startswith("iterations: ") and " converged: 1 " in f32[2] and f32[2] == f64[2]
    assert f32[3] == f64[3] == f"nnz: {np.count_nonzero(A)}"
    assert f32.index("values: float") == 4 and len(f32) == len(f64) + 1
    assert f32[-m:] == f64[-m:]
    x = np.array([float(t) for t in f32[-m:]])
    assert np.linalg.norm(b - A @ x) <= 1e-5 * np.linalg.norm(b)  # x is printed with a few decimals
