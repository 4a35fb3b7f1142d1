"""cgx_set_dia_sym: a one-sided diagonal-valued cgx_create_csr context (k_dia_sym_mult_f64, csrc/cgx_dia_sym.hip) through
every layer.  Everything is stated against the expansion (tests/_dia_sym.py: every stored o > 0 as the two consecutive
full diagonals o, -o), on which k_dia_mult_f64 and a CSR context are already tested:

  1. the kernel's bits against tests/_dia_order.py's CPU statement on the expansion, and against spmv_dia on it, at
     every rows per lane, stored diagonals in flight and load policy;
  2. the grid-stride walk under one block per CU;
  3. contexts: a from_dia_sym solver against a from_dia solver on the expansion, bit for bit -- fixed loops from a rough
     x0, every host form of a converged solve, every preconditioner kind, the preconditioner set-up against a CSR
     context, residual_norm, the fused p.Ap;
  4. the lifecycle, one context through every storage kind, and the refusals; 5. `cg_hip --csr --dia-sym`."""
import functools

import numpy as np
import pytest

import _bsmv_order as bo
import _dia_order as do
import _dia_sym as ds
import _pcg_probe as pp
import conjugate_gradient_amd as cg

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SHAPE = -1, -4
# None on a tree without the feature: every test then fails at its first use
spmv_dia_sym = getattr(cg, "spmv_dia_sym", None)
from_dia_sym = getattr(cg.Solver, "from_dia_sym", None)
DIA_SYM_ACTIVE = getattr(cg, "CGX_DIA_SYM_ACTIVE", None)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert hasattr(cg.Solver, "set_dia_sym"), "the package has no one-sided diagonal storage"


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def no_hip_error():
    assert cg.lib().cgx_hip_last_error() == 0


def code_of(call):
    with pytest.raises(cg.CgxError) as e:
        call()
    return e.value.code, str(e.value)


@functools.lru_cache(maxsize=None)
def banded(n):
    """_pcg_probe.system(n) one-sided (offsets 0, 1, 2, 37) and its expansion; read-only."""
    full = do.from_csr(*pp.system(n).csr(), n)
    offsets, data = ds.upper_of(*full, n)
    assert list(offsets) == [0, 1, 2, 37]
    eo, ed = ds.expand(offsets, data, n)
    assert list(eo) == [0, 1, -1, 2, -2, 37, -37]
    for a in (offsets, data, eo, ed):
        a.setflags(write=False)
    return offsets, data, eo, ed


# ---- 1. kernel bits ----------------------------------------------------------------------------------------------------
def run_kernel(fn, offsets, data, v, n, spare=3):
    dv = cg.DeviceArray.from_host(v)
    dout = cg.DeviceArray.from_host(np.full(n + spare, np.nan))
    fn(offsets, data, dv, dout, n)
    out = dout.to_host()
    dv.free()
    dout.free()
    assert np.isnan(out[n:]).all(), "the kernel stored past the last row"
    return out[:n]


@functools.lru_cache(maxsize=None)
def struct(ndiag):
    """(offsets, data, v, the CPU statement's bits, spmv_dia's bits on the expansion under its default plan)."""
    offsets, data, v = ds.structure_matrix(ndiag)
    eo, ed = ds.expand(offsets, data, ds.STRUCT_N)
    want = do.spmv_dia(eo, ed, v)
    full = run_kernel(cg.spmv_dia, eo, ed, v, ds.STRUCT_N)
    return offsets, data, v, want, full


@pytest.mark.parametrize("R,U,nt", ds.PLANS)
def test_structure_matrix_bits(monkeypatch, R, U, nt):
    monkeypatch.delenv("CGX_DIA_PLAN", raising=False)
    monkeypatch.setenv("CGX_DIA_SYM_PLAN", f"R={R},U={U},nt={nt}")
    for ndiag in ds.STRUCT_NDIAGS:
        offsets, data, v, want, full = struct(ndiag)
        out = run_kernel(spmv_dia_sym, offsets, data, v, ds.STRUCT_N)
        assert same_bits(out, want), (ndiag, R, U, nt, np.flatnonzero(out != want))
        assert same_bits(out, full), (ndiag, R, U, nt)
    no_hip_error()


SMALL_NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def small(n):
    offsets, data, v = ds.small_matrix(n)
    eo, ed = ds.expand(offsets, data, n)
    return offsets, data, v, do.spmv_dia(eo, ed, v), run_kernel(cg.spmv_dia, eo, ed, v, n)


@pytest.mark.parametrize("R,U,nt", ds.PLANS)
def test_small_sizes_bits(monkeypatch, R, U, nt):
    """Offsets {0, 1, 2, n - 1} where they exist; ld = n + 1 is odd at the even sizes (8-byte loads under R = 2) and
    even at the odd ones (16-byte loads); one group, a partial group, two groups and their edges."""
    monkeypatch.delenv("CGX_DIA_PLAN", raising=False)
    monkeypatch.setenv("CGX_DIA_SYM_PLAN", f"R={R},U={U},nt={nt}")
    for n in SMALL_NS:
        offsets, data, v, want, full = small(n)
        out = run_kernel(spmv_dia_sym, offsets, data, v, n)
        assert same_bits(out, want), (n, R, U, nt, np.flatnonzero(out != want))
        assert same_bits(out, full), (n, R, U, nt)
    no_hip_error()


def test_plan_string_naming_no_plan_runs_the_default(monkeypatch):
    offsets, data, v, want, _ = struct(17)
    monkeypatch.delenv("CGX_DIA_SYM_PLAN", raising=False)
    assert same_bits(run_kernel(spmv_dia_sym, offsets, data, v, ds.STRUCT_N), want)
    for plan in ("R=3,U=4,nt=2", "R=1,U=3,nt=2", "R=2,U=4,nt=1", "R=0", "U=16"):
        monkeypatch.setenv("CGX_DIA_SYM_PLAN", plan)
        assert same_bits(run_kernel(spmv_dia_sym, offsets, data, v, ds.STRUCT_N), want)
    no_hip_error()


def test_python_never_launches_on_unchecked_offsets():
    offsets, data, v, _, _ = struct(17)
    dv, dout = cg.DeviceArray.from_host(v), cg.DeviceArray.from_host(np.full(ds.STRUCT_N, np.nan))
    for bad in (ds.STRUCT_N, -1):
        o = offsets.copy()
        o[9] = bad
        with pytest.raises((cg.CgxError, ValueError)):
            spmv_dia_sym(o, data, dv, dout, ds.STRUCT_N)
    assert np.isnan(dout.to_host()).all()  # nothing ran
    dv.free()
    dout.free()


# ---- 2. the grid-stride walk -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ds.RS)
def test_grid_stride_walk(monkeypatch, R):
    """400,003 rows under one block per CU: on 256 CUs a sweep covers 1024 waves x 64 R rows (131,072 at R = 2), so
    every wave walks at least three groups and the last group is partial.  ld = n + 1 is even: 16-byte loads under
    R = 2.  The vector is signed powers of two, so the vectorised CPU statement on the expansion is exact."""
    n = 400003
    offsets = np.array([37, 0, 1, 2, 1000, 4097], np.int32)
    data = ds.mask_unused(offsets, np.random.default_rng(18).standard_normal((offsets.size, n + 1)), n)
    v = bo.pow2_vector(n)
    want = do.spmv_dia_pow2(*ds.expand(offsets, data, n), v)
    monkeypatch.setenv("CGX_DIA_SYM_PLAN", f"R={R},U=4,nt=2,bpc=1")
    out = run_kernel(spmv_dia_sym, offsets, data, v, n)
    assert same_bits(out, want), np.flatnonzero(out != want)[:8]
    no_hip_error()


# ---- 3. contexts -------------------------------------------------------------------------------------------------------
EPS = 1e-9


def fixed_loops(s, b, x0, loops=3):
    """x after each of `loops` fixed-count iterations from x0."""
    s.set_rows(0, b_rows=b, x_rows=x0)
    s.begin()
    out = []
    for _ in range(loops):
        assert s.iterate(1) == (1, False)
        out.append(s.get_x())
    return out


def host_forms(s, b, n, monkeypatch):
    """(loop count, r.r, x) of a converged solve from x0 = 0, the same bits in every host form."""
    monkeypatch.delenv("CGX_GATED", raising=False)
    s.set_rows(0, b_rows=b, x_rows=np.zeros(n))
    x1, st1 = s.solve(x0=np.zeros(n), eps=EPS)  # device-gated
    K = st1.iterations
    assert st1.converged == 1 and 1 < K < 200, (K, st1.converged)
    first = min(3, K - 1)
    monkeypatch.setenv("CGX_GATED", "0")  # host-checked convergence
    x2, st2 = s.solve(x0=np.zeros(n), eps=EPS)
    assert same_bits(x2, x1) and (st2.iterations, st2.converged, st2.rr) == (K, 1, st1.rr)
    monkeypatch.delenv("CGX_GATED")
    s.set_x(np.zeros(n))  # fixed count
    s.begin()
    assert s.iterate(K) == (K, False)
    assert same_bits(s.get_x(), x1) and s.stats().rr == st1.rr
    s.set_x(np.zeros(n))  # in pieces
    s.begin()
    assert s.iterate(first) == (first, False)
    done, conv = s.iterate(1000, eps=EPS)
    assert (first + done, conv) == (K, True)
    assert same_bits(s.get_x(), x1) and s.stats().iterations == K and s.stats().rr == st1.rr
    return K, st1.rr, x1


def preconds(n, sd):
    """(name, how to set it on a solver): plain and every preconditioner kind.  The caller's blocks are the library's
    own inverses for pbs = 3 (symmetric positive definite, so the solve converges), handed back as values."""
    sd.set_precond(("block", 3))
    W3 = sd.precond_block[1].copy()
    sd.set_precond(None)
    out = [("plain", lambda s: s.set_precond(None)),
           ("jacobi", lambda s: s.set_precond("jacobi")),
           ("minv", lambda s: s.set_precond(pp.minv(n, "diag")))]
    out += [(f"block {pbs}", lambda s, pbs=pbs: s.set_precond(("block", pbs))) for pbs in (2, 3, 8)]
    out.append(("block values", lambda s: s.set_precond_block(3, values=W3)))
    return out


@pytest.mark.parametrize("n", [38, 257, 2049])
def test_context_against_full_dia_on_the_expansion(monkeypatch, n):
    sys_ = pp.system(n)
    offsets, data, eo, ed = banded(n)
    with from_dia_sym(offsets, data) as ss, cg.Solver.from_dia(eo, ed, n=n) as sd, \
            cg.Solver.from_csr(*do.expand(eo, ed, n)) as sc:
        f = ss.info.flags
        assert f & DIA_SYM_ACTIVE and f & cg.CGX_DIA_ACTIVE and f & cg.CGX_CSR_ACTIVE and not f & cg.CGX_BSR_ACTIVE
        assert not sd.info.flags & DIA_SYM_ACTIVE
        assert ss.csr_nnz == 4 * n < sd.csr_nnz == 7 * n  # half the room
        for name, setp in preconds(n, sd):
            for s in (ss, sd, sc):
                setp(s)
            # the set-up's bits against a CSR context on the expansion
            if name in ("jacobi", "minv"):
                assert same_bits(ss.precond_diag(), sc.precond_diag()), name
                if name == "jacobi":
                    assert same_bits(ss.precond_diag(), 1.0 / sys_.diag)
            elif name.startswith("block"):
                (gs, Ws), (gc, Wc) = ss.precond_block, sc.precond_block
                assert gs == gc and same_bits(Ws, Wc), name
            for R, U, nt in ((1, 1, 8), (2, 4, 2), (2, 8, 8), (1, 2, 2)):
                for s in (ss, sd):
                    s.set_matvec_plan(64 * R, U, nt)
                ps, pd = ss.matvec_plan(), sd.matvec_plan()
                assert ps == pd and (ps["R"], ps["U"], ps["nt"]) == (64 * R, U, nt), (ps, pd)  # the same grid too
                # three fixed loops from a rough x0: the matVec's rows and the fused p.Ap (x after the first loop)
                xs, xd = fixed_loops(ss, sys_.b, sys_.x0), fixed_loops(sd, sys_.b, sys_.x0)
                for k, (a, b) in enumerate(zip(xs, xd)):
                    assert np.isfinite(a).all() and same_bits(a, b), (name, R, U, nt, k)
                rs, rd = ss.residual_norm(), sd.residual_norm()
                assert rs == rd and rs[0] > 0.0, (name, rs, rd)
            got = [host_forms(s, sys_.b, n, monkeypatch) for s in (ss, sd)]
            assert got[0][:2] == got[1][:2] and same_bits(got[0][2], got[1][2]), (name, got[0][:2], got[1][:2])
            A = sys_.dense()
            assert np.linalg.norm(sys_.b - A @ got[0][2]) <= 1e-8 * np.linalg.norm(sys_.b)
    no_hip_error()


def scrambled(n, seed=4):
    """banded(n) one-sided with the diagonals unsorted, offset 0 stored twice in two pieces that sum to the diagonal
    only in the stored order, and offset 1 twice; NaN in the unused slots."""
    offsets, data, _, _ = banded(n)
    by = {int(o): data[k] for k, o in enumerate(offsets)}
    a = np.random.default_rng([seed, n]).standard_normal(n)
    c = np.random.default_rng([seed, n, 1]).standard_normal(n)
    order = (37, 0, 1, 2, 0, 1)
    rows, first0, first1 = [], True, True
    for o in order:
        if o == 0:
            rows.append(by[0] + a if first0 else -a)
            first0 = False
        elif o == 1:
            rows.append(by[1] + c if first1 else -c)
            first1 = False
        else:
            rows.append(by[o].copy())
    return np.array(order, np.int32), ds.mask_unused(order, np.array(rows), n)


def test_precond_setup_bits_on_an_unsorted_matrix_with_duplicates():
    n = 257
    offsets, data = scrambled(n)
    eo, ed = ds.expand(offsets, data, n)
    csr = do.expand(eo, ed, n)
    assert np.isfinite(csr[2]).all()
    with from_dia_sym(offsets, data) as ss, cg.Solver.from_csr(*csr) as sc:
        ss.set_precond("jacobi")
        sc.set_precond("jacobi")
        assert same_bits(ss.precond_diag(), sc.precond_diag())
        assert not same_bits(ss.precond_diag(), 1.0 / pp.system(n).diag)  # the two pieces do round
        for pbs in range(2, 9):
            ss.set_precond_block(pbs)
            sc.set_precond_block(pbs)
            (gs, Ws), (gc, Wc) = ss.precond_block, sc.precond_block
            assert gs == gc == pbs and same_bits(Ws, Wc), pbs
    # no diagonal of offset 0: CSR's failure, the earlier preconditioner stays
    o2, d2, _, _ = banded(n)
    with from_dia_sym(o2[1:], d2[1:], n=n) as sm:
        sm.set_precond(np.full(n, 0.5))
        code, msg = code_of(lambda: sm.set_precond("jacobi"))
        assert code == ERR_SHAPE and "row 0 has no diagonal entry" in msg, msg
        assert code_of(lambda: sm.set_precond_block(3))[0] == ERR_SHAPE
        assert sm.precond == "diag" and same_bits(sm.precond_diag(), np.full(n, 0.5))
    no_hip_error()


# ---- 4. lifecycle and refusals -----------------------------------------------------------------------------------------
def solve0(s, n):
    x, st = s.solve(x0=np.zeros(n), eps=EPS)
    return x, st.iterations, st.rr


def test_lifecycle_and_failed_calls():
    n = 257
    sys_ = pp.system(n)
    csr = sys_.csr()
    offsets, data, eo, ed = banded(n)
    ndiag, cap = offsets.size, offsets.size * n
    L = cg.lib()
    err = lambda: L.cgx_last_error().decode()  # noqa: E731
    o, d = np.ascontiguousarray(offsets), np.ascontiguousarray(data)
    po, pd = o.ctypes.data, d.ctypes.data
    bad_o = o.copy()
    bad_o[2] = -2
    big_o = o.copy()
    big_o[3] = n

    def failed_calls(s):
        """Every refusal of cgx_set_dia_sym, in cgx_set_dia's order."""
        assert L.cgx_set_dia_sym(None, ndiag, po, pd, n) == ERR_ARG and "ctx is NULL" in err()
        assert L.cgx_set_dia_sym(s._h, -1, po, pd, n) == ERR_ARG and "ndiag" in err()
        assert L.cgx_set_dia_sym(s._h, ndiag, None, pd, n) == ERR_ARG and "NULL" in err()
        assert L.cgx_set_dia_sym(s._h, ndiag, po, None, n) == ERR_ARG and "NULL" in err()
        assert L.cgx_set_dia_sym(s._h, ndiag, po, pd, n - 1) == ERR_SHAPE and "ld = 256" in err() and "n = 257" in err()
        # ld comes before the capacity, the capacity before the offsets
        over = cap // n + 1  # one stored diagonal more than the context has room for
        more_o, more_d = np.resize(bad_o, over), np.ascontiguousarray(np.resize(d, (over, n)))
        assert L.cgx_set_dia_sym(s._h, over, more_o.ctypes.data, more_d.ctypes.data, n - 1) == ERR_SHAPE
        assert "ld = 256" in err()
        assert L.cgx_set_dia_sym(s._h, over, more_o.ctypes.data, more_d.ctypes.data, n) == ERR_SHAPE
        assert "room for" in err() and str(cap) in err() and str(over * n) in err()
        assert L.cgx_set_dia_sym(s._h, 2 ** 62, po, pd, n) == ERR_SHAPE and "room for" in err()  # no overflow
        assert L.cgx_set_dia_sym(s._h, ndiag, bad_o.ctypes.data, pd, n) == ERR_SHAPE
        assert "cgx_dia_sym_check" in err() and "offsets[2] = -2" in err() and "offsets >= 0" in err()
        assert L.cgx_set_dia_sym(s._h, ndiag, big_o.ctypes.data, pd, n) == ERR_SHAPE and f"offsets[3] = {n}" in err()
        assert code_of(lambda: s.set_dia_sym(bad_o, d))[0] == ERR_SHAPE

    with cg.Solver.from_csr(*csr) as fresh:
        fresh.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        want_c, plan_c = solve0(fresh, n), fresh.matvec_plan()
    with cg.Solver(n, csr_nnz=cap) as s:  # room for the stored diagonals, not for the expansion
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        # the expansion through set_dia does not fit
        assert L.cgx_set_dia(s._h, eo.size, np.ascontiguousarray(eo).ctypes.data, np.ascontiguousarray(ed).ctypes.data,
                             n) == ERR_SHAPE and "room for" in err()
        # one-sided: the flags, a default plan
        s.set_dia_sym(offsets, data)
        f = s.info.flags
        assert f & DIA_SYM_ACTIVE and f & cg.CGX_DIA_ACTIVE and f & cg.CGX_CSR_ACTIVE and not f & cg.CGX_BSR_ACTIVE
        default = s.matvec_plan()
        xs = solve0(s, n)
        assert rel(xs[0], want_c[0]) <= 1e-8
        # plan refusals: the plan stays
        for bad in ((32, 4, 2), (192, 4, 2), (64, 3, 2), (64, 16, 2), (64, 0, 2), (128, 4, 1), (128, 4, 0), (8, 1, 2)):
            code, msg = code_of(lambda: s.set_matvec_plan(*bad))
            assert code == ERR_ARG and s.matvec_plan() == default, (bad, msg)
        # a plan the caller chose on a one-sided context survives the next set_dia_sym
        s.set_matvec_plan(128, 2, 2)
        s.set_dia_sym(offsets, data)
        pl = s.matvec_plan()
        assert (pl["R"], pl["U"], pl["nt"]) == (128, 2, 2)
        # from one-sided: a failed call keeps the one-sided matrix, its plan, preconditioner and bits
        s.set_precond(("block", 2))
        before = solve0(s, n)
        failed_calls(s)
        assert s.info.flags & DIA_SYM_ACTIVE and s.matvec_plan() == pl and s.precond == "block"
        after = solve0(s, n)
        assert same_bits(after[0], before[0]) and after[1:] == before[1:]
        # a successful call turns preconditioning off
        s.set_dia_sym(offsets, data)
        assert s.precond == "none" and not s.info.flags & cg.CGX_PRECOND_ACTIVE
        # the zero matrix is a matrix
        s.set_dia_sym(np.zeros(0, np.int32), np.zeros((0, n)))
        assert s.info.flags & DIA_SYM_ACTIVE
        assert L.cgx_set_dia_sym(s._h, 0, None, None, n) == 0
    cap = eo.size * n  # room for the CSR arrays and the expansion from here on
    with cg.Solver(n, csr_nnz=cap) as s:
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        # from CSR: a failed call keeps the CSR matrix, its preconditioner and its bits
        s.set_csr(*csr)
        s.set_precond("jacobi")
        before = solve0(s, n)
        failed_calls(s)
        f = s.info.flags
        assert f & cg.CGX_CSR_ACTIVE and not f & cg.CGX_DIA_ACTIVE and not f & DIA_SYM_ACTIVE
        assert s.precond == "jacobi" and s.matvec_plan() == plan_c
        after = solve0(s, n)
        assert same_bits(after[0], before[0]) and after[1:] == before[1:]
        # CSR -> one-sided -> CSR: a fresh CSR context's bits and a default plan
        s.set_dia_sym(offsets, data)
        assert s.info.flags & DIA_SYM_ACTIVE and s.precond == "none" and s.matvec_plan() == default
        s.set_csr(*csr)
        f = s.info.flags
        assert f & cg.CGX_CSR_ACTIVE and not f & cg.CGX_DIA_ACTIVE and not f & DIA_SYM_ACTIVE
        assert s.matvec_plan() == plan_c and s.precond == "none"
        got = solve0(s, n)
        assert same_bits(got[0], want_c[0]) and got[1:] == want_c[1:]
    # from DIA, on a context with room for the expansion: a failed call keeps the diagonal matrix; a plan chosen on
    # the full kind does not carry over to the one-sided kind, nor back
    with cg.Solver.from_dia(eo, ed, n=n) as fresh:
        fresh.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        want_d, plan_d = solve0(fresh, n), fresh.matvec_plan()
    with cg.Solver(n, csr_nnz=eo.size * n) as s:
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        s.set_dia(eo, ed)
        failed_calls(s)
        f = s.info.flags
        assert f & cg.CGX_DIA_ACTIVE and not f & DIA_SYM_ACTIVE and s.matvec_plan() == plan_d
        got = solve0(s, n)
        assert same_bits(got[0], want_d[0]) and got[1:] == want_d[1:]
        s.set_matvec_plan(128, 4, 2)
        s.set_dia_sym(offsets, data)
        assert s.matvec_plan() == default and s.info.flags & DIA_SYM_ACTIVE
        s.set_matvec_plan(128, 4, 2)
        s.set_dia(eo, ed)
        f = s.info.flags
        assert f & cg.CGX_DIA_ACTIVE and not f & DIA_SYM_ACTIVE and s.matvec_plan() == plan_d
        got = solve0(s, n)
        assert same_bits(got[0], want_d[0]) and got[1:] == want_d[1:]
    no_hip_error()


def transition_matrix(n=38):
    """A symmetric, diagonally dominant matrix of small integers that fits a context with room for 5 n entries in
    every storage: one-sided offsets (0, 1, 37), so the expansion (0, 1, -1, 37, -37) is 5 diagonals; the couplings
    (i, i + 1) between two 2 x 2 blocks are zero except at i = 1 mod 4, so bs = 2 stores 39 blocks (156 entries).
    With p of signed powers of two every product and every partial sum of A p, p.p and p.Ap is an integer below
    2^53: the bits depend on no summation order, and one statement serves the CSR, BSR and diagonal kernels."""
    i = np.arange(n)
    data = np.zeros((3, n))
    data[0] = 16.0
    data[1, 1:] = np.where((i[:-1] % 2 == 0) | (i[:-1] % 4 == 1), (i[:-1] % 3) - 3.0, 0.0)  # A[i][i + 1] at slot i + 1
    data[2, 37:] = 2.0
    offsets = np.array([0, 1, 37], np.int32)
    eo, ed = ds.expand(offsets, ds.mask_unused(offsets, data, n), n)
    A = do.dense(eo, np.nan_to_num(ed), n)
    assert np.array_equal(A, A.T) and np.count_nonzero(A) <= 5 * n
    rows, cols = np.nonzero(A)
    csr = (np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64), cols.astype(np.int32),
           A[rows, cols])
    bsr = bo.from_dense(A, 2)
    assert bsr[2].size <= 5 * n
    p = np.where(i % 3 == 0, -1.0, 1.0) * 2.0 ** (i % 4)
    return offsets, ds.mask_unused(offsets, data, n), eo, ed, csr, bsr, p


def test_storage_transitions_on_one_context(monkeypatch):
    """One context through every storage kind: after each upload the plan, the storage flags and the matVec.  A plan
    the caller chose carries over exactly between CSR and BSR (T and the policy; the grid follows the rows) and is
    dropped by every step that enters or leaves a diagonal kind or switches between the two.  The expected plans are
    the plan rules' on this matrix (CSR: mean row length 2, T = 2; a diagonal kind's defaults; n = 38 is one group
    of a diagonal kernel and one block), the same on the commit before the kinds shared one upload tail.
    The context hands out neither A p nor p.Ap, so: A p through residual_norm with x = p and b = the CPU statement's
    A p on the expansion (||b - A x|| is 0.0 exactly when every row has its value; this launch has no fused dot), and
    the fused p.Ap through one iteration from x0 = 0 with b = p, where x_1 = fl(p.p / p.Ap) p bit for bit."""
    for env in ("CGX_SPMV_PLAN", "CGX_BSMV_PLAN", "CGX_DIA_PLAN", "CGX_DIA_SYM_PLAN", "CGX_GATED"):
        monkeypatch.delenv(env, raising=False)
    n = 38
    offsets, data, eo, ed, csr, bsr, p = transition_matrix(n)
    Ap = do.spmv_dia(eo, ed, p)
    assert same_bits(Ap, do.dense(eo, np.nan_to_num(ed), n) @ p) and float(p @ Ap) > 0.0  # exact in any order
    x1 = (float(p @ p) / float(p @ Ap)) * p
    BSR, DIA, SYM = cg.CGX_BSR_ACTIVE, cg.CGX_DIA_ACTIVE, DIA_SYM_ACTIVE
    plan = lambda R, U, nt, blocks: dict(R=R, U=U, nt=nt, blocks=blocks)  # noqa: E731
    steps = (
        ("set_csr", lambda s: s.set_csr(*csr), plan(32, 1, 2, 1), 0),
        ("set_matvec_plan (CSR)", lambda s: s.set_matvec_plan(8, 1, 8), plan(8, 1, 8, 2), 0),
        ("set_bsr", lambda s: s.set_bsr(*bsr), plan(8, 1, 8, 1), BSR),  # T = 8 and policy 8 kept, 19 block rows
        ("set_dia", lambda s: s.set_dia(eo, ed), plan(64, 1, 8, 1), DIA),  # dropped: the full kind's default
        ("set_matvec_plan (DIA)", lambda s: s.set_matvec_plan(128, 4, 2), plan(128, 4, 2, 1), DIA),
        ("set_dia_sym", lambda s: s.set_dia_sym(offsets, data), plan(128, 8, 2, 1), DIA | SYM),  # dropped
        ("set_dia", lambda s: s.set_dia(eo, ed), plan(64, 1, 8, 1), DIA),
        ("set_csr_f32", lambda s: s.set_csr(*csr, a_f32=True), plan(32, 1, 2, 1), 0),
        ("set_csr", lambda s: s.set_csr(*csr), plan(32, 1, 2, 1), 0),
    )
    with cg.Solver(n, csr_nnz=5 * n) as s:
        for k, (name, step, want_plan, want_flags) in enumerate(steps):
            step(s)
            assert s.matvec_plan() == want_plan, (k, name, s.matvec_plan())
            assert s.info.flags & (BSR | DIA | SYM) == want_flags, (k, name, hex(s.info.flags))
            assert bool(s.info.flags & cg.CGX_A_F32) == (name == "set_csr_f32"), (k, name)
            s.set_rows(0, b_rows=Ap, x_rows=p)
            assert s.residual_norm() == (0.0, float(np.sqrt(Ap @ Ap))), (k, name, s.residual_norm())
            s.set_rows(0, b_rows=p, x_rows=np.zeros(n))
            s.begin()
            assert s.iterate(1) == (1, False)
            got = s.get_x()
            assert same_bits(got, x1), (k, name, np.flatnonzero(got != x1))
    no_hip_error()


def test_set_dia_sym_refused_on_other_contexts():
    offsets, data, _, _ = banded(258)
    o, d = np.ascontiguousarray(offsets), np.ascontiguousarray(data)
    L = cg.lib()
    args = (o.size, o.ctypes.data, d.ctypes.data, 258)
    nnz = 7 * 258
    csr = pp.system(258).csr()
    for with_matrix in (False, True):
        with cg.Solver.csr(258, nnz, nrhs=2) as s:
            if with_matrix:
                s.set_csr(*csr)
            assert L.cgx_set_dia_sym(s._h, *args) == ERR_ARG
            assert "right-hand sides" in L.cgx_last_error().decode() and "not built" in L.cgx_last_error().decode()
            with pytest.raises(ValueError):
                s.set_dia_sym(offsets, data)
        with cg.Solver.csr(258, nnz, devices=[0, 0]) as s:
            if with_matrix:
                s.set_csr(*csr)
            assert L.cgx_set_dia_sym(s._h, *args) == ERR_ARG
            assert "row blocks" in L.cgx_last_error().decode() and "not built" in L.cgx_last_error().decode()
            with pytest.raises(ValueError):
                s.set_dia_sym(offsets, data)
    with cg.Solver.csr(258, nnz, devices=[0]) as s:
        assert L.cgx_set_dia_sym(s._h, *args) == ERR_ARG
    with cg.Solver(258) as s:
        assert L.cgx_set_dia_sym(s._h, *args) == ERR_ARG
        assert "not a cgx_create_csr context" in L.cgx_last_error().decode()
    no_hip_error()


# ---- 5. CLI ------------------------------------------------------------------------------------------------------------
def test_cli_dia_sym(tmp_path):
    import os
    import subprocess

    import oracle
    one_gpu = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    n = 130
    sys_ = pp.system(n)
    for name, arr, dec in (("A.txt", sys_.dense(), 6), ("b.txt", sys_.b, 9), ("x0.txt", np.zeros(n), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    Aw = cg.read_text(paths[0], n * n, np.float64).reshape(n, n)  # the matrix as the file holds it
    bw = cg.read_text(paths[1], n, np.float64)
    assert np.array_equal(Aw, Aw.T)

    def run(*opts):
        r = subprocess.run([cg.CLI_PATH, *opts, "--eps", "1e-12", "--print-x", "--stats", *paths],
                           capture_output=True, text=True, timeout=300, env=one_gpu)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().splitlines()
        return lines[:-n], np.array([float(v) for v in lines[-n:]])

    for extra, label in (((), None), (("--jacobi",), "precond: jacobi"), (("--block-jacobi", "4"), "precond: block-jacobi 4")):
        head_d, x_d = run("--csr", "--dia", *extra)
        head_s, x_s = run("--csr", "--dia-sym", *extra)
        assert head_s[0] == head_d[0] == f"Computing cg of matrix size : {n * n}"
        assert head_s[2].startswith("iterations: ") and " converged: 1 " in head_s[2], head_s[2]
        assert head_s[2].split(" residual_norm")[0] == head_d[2].split(" residual_norm")[0]  # the same converged line
        assert head_s[3] == head_d[3] and head_d[4] == "ndiag: 7" and head_s[4] == "ndiag: 4"
        assert len(head_s) == len(head_d) and (label is None or head_s[5] == head_d[5] == label)
        assert rel(x_s, x_d) <= 1e-8
        assert np.linalg.norm(bw - Aw @ x_s) <= 1e-10 * np.linalg.norm(bw)
    # one lower entry changed: the run ends and names it
    i, j = 41, 4
    assert Aw[i, j] != 0.0
    B = Aw.copy()
    B[i, j] += 0.5
    oracle.write_text(str(tmp_path / "B.txt"), B, 6)
    r = subprocess.run([cg.CLI_PATH, "--csr", "--dia-sym", str(tmp_path / "B.txt"), *paths[1:]], capture_output=True,
                       text=True, timeout=300, env=one_gpu)
    assert r.returncode != 0 and r.stderr.startswith("--dia-sym:") and f"({i}, {j})" in r.stderr, r.stderr
    for opts in (("--dia-sym",), ("--csr-a32", "--dia-sym"), ("--csr", "--dia-sym", "--bsr", "2"),
                 ("--csr", "--dia", "--dia-sym")):
        r = subprocess.run([cg.CLI_PATH, *opts, *paths], capture_output=True, text=True, timeout=60, env=one_gpu)
        assert r.returncode != 0 and r.stderr.startswith("--dia-sym holds a --csr matrix by its upper diagonals"), \
            (opts, r.stderr)
