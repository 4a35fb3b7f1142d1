"""cgx_set_dia: a diagonal-valued cgx_create_csr context (k_dia_mult_f64, csrc/cgx_dia.hip) through every layer.

  1. the kernel's bits against the CPU statement of its summation order (tests/_dia_order.py) at every rows per lane,
     diagonals in flight and load policy, kernel-level and through a context;
  2. the grid-stride walk under one block per CU;
  3. the element-wise probe of the iteration, plain and under every preconditioner kind, against the long-double
     references and bars of tests/_nrhs_probe.py and tests/_pcg_probe.py (tests/test_dia_cpu.py asserts that those
     bars are reachable at these sizes);
  4. the host forms; 5. converged solves against a CSR context on the expansion; 6. the preconditioner set-up's bits
     against a CSR context on the expanded matrix; 7. the fused p.Ap; 8. the lifecycle and the refusals; 9. `cg_hip --csr --dia`.

The probe's matrix is ``_pcg_probe.system(n)`` held as its 7 diagonals, offsets ascending, zero-filled."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import _bsmv_order as bo
import _dia_order as do
import _nrhs_probe as npr
import _pcg_probe as pp
import conjugate_gradient_amd as cg

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SHAPE = -1, -4
LD = np.longdouble
# None on a tree without the feature: every test then fails at its first use
spmv_dia = getattr(cg, "spmv_dia", None)
from_dia = getattr(cg.Solver, "from_dia", None)
DIA_ACTIVE = getattr(cg, "CGX_DIA_ACTIVE", None)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert hasattr(cg.Solver, "set_dia"), "the package has no diagonal storage"


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
def banded_dia(n):
    """_pcg_probe.system(n) as 7 diagonals, offsets ascending, zero-filled; read-only."""
    out = do.from_csr(*pp.system(n).csr(), n)
    assert list(out[0]) == [-37, -2, -1, 0, 1, 2, 37]
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. order ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def struct(ndiag):
    offsets, data, v = do.structure_matrix(ndiag)
    return offsets, data, v, do.spmv_dia(offsets, data, v)


def run_kernel(offsets, data, v, n, spare=3):
    dv = cg.DeviceArray.from_host(v)
    dout = cg.DeviceArray.from_host(np.full(n + spare, np.nan))
    spmv_dia(offsets, data, dv, dout, n)
    out = dout.to_host()
    dv.free()
    dout.free()
    assert np.isnan(out[n:]).all(), "the kernel stored past the last row"
    return out[:n]


@pytest.mark.parametrize("R,U,nt", do.PLANS)
def test_structure_matrix_bits(monkeypatch, R, U, nt):
    monkeypatch.setenv("CGX_DIA_PLAN", f"R={R},U={U},nt={nt}")
    for ndiag in do.STRUCT_NDIAGS:
        offsets, data, v, want = struct(ndiag)
        out = run_kernel(offsets, data, v, do.STRUCT_N)
        assert same_bits(out, want), (ndiag, R, U, nt, np.flatnonzero(out != want))
    no_hip_error()


SMALL_NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def small(n):
    offsets, data, v = do.small_matrix(n)
    return offsets, data, v, do.spmv_dia(offsets, data, v)


@pytest.mark.parametrize("R,U,nt", [(R, U, nt) for R, U, nt in do.PLANS if (U, nt) in ((1, 8), (4, 2), (8, 2))])
def test_small_sizes_bits(monkeypatch, R, U, nt):
    """Offsets {0, +-1, +-2, +-(n-1)} where they exist; ld = n + 1 is odd at the even sizes (8-byte loads under
    R = 2) and even at the odd ones (16-byte loads)."""
    monkeypatch.setenv("CGX_DIA_PLAN", f"R={R},U={U},nt={nt}")
    for n in SMALL_NS:
        offsets, data, v, want = small(n)
        out = run_kernel(offsets, data, v, n)
        assert same_bits(out, want), (n, R, U, nt, np.flatnonzero(out != want))
    no_hip_error()


def test_plan_string_naming_no_plan_runs_the_default(monkeypatch):
    offsets, data, v, want = struct(17)
    monkeypatch.delenv("CGX_DIA_PLAN", raising=False)
    assert same_bits(run_kernel(offsets, data, v, do.STRUCT_N), want)
    for plan in ("R=3,U=4,nt=2", "R=1,U=3,nt=2", "R=2,U=4,nt=1", "R=0", "U=16"):
        monkeypatch.setenv("CGX_DIA_PLAN", plan)
        assert same_bits(run_kernel(offsets, data, v, do.STRUCT_N), want)
    no_hip_error()


def test_python_never_launches_on_unchecked_offsets():
    offsets, data, v, _ = struct(17)
    dv, dout = cg.DeviceArray.from_host(v), cg.DeviceArray.from_host(np.full(do.STRUCT_N, np.nan))
    for bad in (do.STRUCT_N, -do.STRUCT_N):
        o = offsets.copy()
        o[9] = bad
        with pytest.raises((cg.CgxError, ValueError)):
            spmv_dia(o, data, dv, dout, do.STRUCT_N)
    assert np.isnan(dout.to_host()).all()  # nothing ran


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("ndiag", [5, 9, 17])
def test_structure_matrix_bits_through_a_context(ndiag):
    """A context's matVec, read back through one fixed loop from x0 = v with b = 0: r_0 = 0 - A v exactly, p_0 = r_0,
    and x_1[i] = fma(alpha, p_0[i], v[i]) with the one alpha of the loop.  With w = the emulation's A v, some double
    alpha within a few ulp of (v[i] - x_1[i]) / w[i] must give every element of x_1 bit for bit; a w that differs
    from the kernel's in one bit of one row has none.  (The matrix need not be SPD for one fixed loop.)"""
    offsets, data, v, w = struct(ndiag)
    n = do.STRUCT_N
    with from_dia(offsets, data, n=n) as s:
        assert s.info.flags & DIA_ACTIVE and s.info.flags & cg.CGX_CSR_ACTIVE
        assert not s.info.flags & cg.CGX_BSR_ACTIVE
        for R, U, nt in do.PLANS:
            s.set_matvec_plan(64 * R, U, nt)
            pl = s.matvec_plan()
            assert (pl["R"], pl["U"], pl["nt"]) == (64 * R, U, nt)
            s.set_rows(0, b_rows=np.zeros(n), x_rows=v)
            s.begin()
            assert s.iterate(1) == (1, False)
            x1 = s.get_x()
            assert np.isfinite(x1).all()
            # the row where alpha w weighs most against x: the least cancellation in v - x_1
            i0 = int(np.argmax(np.abs(w) / np.maximum(np.abs(v), np.abs(x1))))
            guess = (v[i0] - x1[i0]) / w[i0]
            cands = [guess]
            for _ in range(64):
                cands = [np.nextafter(cands[0], -np.inf)] + cands + [np.nextafter(cands[-1], np.inf)]
            hit = [a for a in cands if all(fma(a, -w[i], v[i]) == x1[i] for i in range(n))]
            assert hit, (ndiag, R, U, nt)
    no_hip_error()


# ---- 2. the grid-stride walk -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", do.RS)
def test_grid_stride_walk(monkeypatch, R):
    """300,001 rows under one block per CU: on 256 CUs a sweep covers 1024 waves x 64 R rows (65,536 / 131,072), so a
    wave walks several groups and the last group is partial.  ld = n + 1 is even: 16-byte loads under R = 2."""
    n = 300001
    offsets = np.array([-37, -1, 0, 1, 2, 1000], np.int32)
    data = np.random.default_rng(17).standard_normal((offsets.size, n + 1))
    for k, o in enumerate(offsets):
        lo, hi = do.in_range(int(o), n)
        data[k, :lo] = np.nan
        data[k, hi:] = np.nan
    v = do.pow2_vector(n)
    want = do.spmv_dia_pow2(offsets, data, v)
    monkeypatch.setenv("CGX_DIA_PLAN", f"R={R},U=4,nt=2,bpc=1")
    out = run_kernel(offsets, data, v, n)
    assert same_bits(out, want), np.flatnonzero(out != want)[:8]
    no_hip_error()


# ---- 3. the element-wise probe of the iteration ------------------------------------------------------------------------
def snapshots(s):
    """(x, r.r) after each of the loops 1, 2, 3 of a fixed-count solve from the context's b and x."""
    s.begin()
    out = []
    for _ in pp.KS:
        assert s.iterate(1) == (1, False)
        out.append((s.get_x(), s.stats().rr))
    return out


def run_probe(s, b, x0, refs, what):
    """refs[k] = (x_ld, S, bar) and optionally (rr_ld, T, rr_bar): every element of x (and r.r) after every loop to
    the bar, then the bits of a second run and of the one-call form."""
    s.set_rows(0, b_rows=b, x_rows=x0)
    snaps = snapshots(s)
    worst, bad = {}, []
    for k, (x, rr) in zip(pp.KS, snaps):
        x_ld, S, bar = refs[k][:3]
        q = pp.ratios(x, x_ld, S).astype(np.float64) / bar
        worst[k] = float(np.max(q))
        if not np.all(q <= 1.0):  # NaN included
            rows = np.flatnonzero(~(q <= 1.0))
            bad.append((k, "x", rows.size, [(int(i), float(q[i])) for i in rows[:8]]))
        if len(refs[k]) > 3 and refs[k][3] is not None:
            rr_ld, T, rr_bar = refs[k][3:]
            qr = float(abs(LD(rr) - rr_ld) / T) / rr_bar
            worst[k] = max(worst[k], qr)
            if not qr <= 1.0:
                bad.append((k, "r.r", qr))
    print(f"\n[dia probe] {what}: " + ", ".join(f"k={k} {v:.3g} of the bar" for k, v in worst.items()))
    assert not bad, (what, bad)
    s.set_rows(0, x_rows=x0)
    again = snapshots(s)
    assert all(same_bits(a[0], x[0]) and a[1] == x[1] for a, x in zip(again, snaps))
    x3, st = s.solve(x0=x0, eps=-1.0, max_iter=max(pp.KS))
    assert st.iterations == max(pp.KS) and same_bits(x3, snaps[-1][0])


@pytest.mark.parametrize("n", [257, 2049])
def test_iteration_probe(n):
    sys_ = pp.system(n)
    with from_dia(*banded_dia(n)) as s:
        assert s.info.flags & DIA_ACTIVE
        for zero in (False, True):
            tag = f"n {n} x0 {'0' if zero else 'rough'}"
            # plain CG: _nrhs_probe's column 0 of the same banded system
            col = npr.Col("csr", n, 0, zero)
            ref = npr.column(col)
            b, x0 = npr.start(col)
            s.set_precond(None)
            run_probe(s, b, x0, {k: (ref.X[k], ref.S[k], npr.bar(col, k),
                                     *((ref.RR[k], ref.T[k], npr.rr_bar(col, k)) if k in npr.rr_loops(n) else (None,)))
                                 for k in pp.KS}, "plain " + tag)
            # the preconditioned kinds: _pcg_probe's b and x0
            x0 = np.zeros(n) if zero else sys_.x0
            for kind, pbs in (("jacobi", 0), ("diag", 0), ("block", 2), ("block", 8)):
                case = pp.Case(kind, pbs, n, zero)
                if kind == "block":
                    s.set_precond_block(pbs, values=pp.blocks(n, pbs)[1])
                else:
                    s.set_precond(pp.library_precond(case))
                assert s.precond == kind
                if kind == "jacobi":  # extracted from the diagonals: 1 / diag(A) bit for bit
                    assert same_bits(s.precond_diag(), 1.0 / sys_.diag)
                pr = pp.probe(case)
                run_probe(s, sys_.b, x0, {k: (pr.X[k], pr.S[k], pp.bar(case, k)) for k in pp.KS},
                          f"{kind} {pbs or ''} " + tag)
    no_hip_error()


# ---- 4. host forms -----------------------------------------------------------------------------------------------------
def test_host_forms(monkeypatch):
    n = 2049
    sys_ = pp.system(n)
    eps = 1e-9
    monkeypatch.delenv("CGX_GATED", raising=False)
    with from_dia(*banded_dia(n)) as s:
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        x1, st1 = s.solve(x0=np.zeros(n), eps=eps)  # device-gated
        K = st1.iterations
        assert st1.converged == 1 and 3 < K < 200
        assert s.iterate(10, eps=eps) == (0, True)  # nothing after convergence
        # in pieces
        s.set_x(np.zeros(n))
        s.begin()
        assert s.iterate(3) == (3, False)
        done, conv = s.iterate(1000, eps=eps)
        assert (3 + done, conv) == (K, True)
        assert same_bits(s.get_x(), x1) and s.stats().iterations == K and s.stats().rr == st1.rr
        # fixed count
        s.set_x(np.zeros(n))
        s.begin()
        assert s.iterate(K) == (K, False)
        assert same_bits(s.get_x(), x1) and s.stats().rr == st1.rr
        # host-checked convergence
        monkeypatch.setenv("CGX_GATED", "0")
        x3, st3 = s.solve(x0=np.zeros(n), eps=eps)
        assert same_bits(x3, x1) and (st3.iterations, st3.converged, st3.rr) == (K, 1, st1.rr)
        monkeypatch.delenv("CGX_GATED")
        rn, bn = s.residual_norm()  # the diagonal kernel again
        A = sys_.dense()
        assert abs(rn - np.linalg.norm(sys_.b - A @ x1)) <= 1e-12 * np.linalg.norm(sys_.b)
        assert abs(bn - np.linalg.norm(sys_.b)) <= 1e-12 * np.linalg.norm(sys_.b)
    no_hip_error()


# ---- 5. converged solves -----------------------------------------------------------------------------------------------
def poisson_dia(m):
    """The 5-point Poisson matrix of an m x m grid as 5 diagonals (the +-1 diagonals hold stored zeros where a grid
    row ends)."""
    n = m * m
    j = np.arange(n)
    offsets = np.array([-m, -1, 0, 1, m], np.int32)
    data = np.zeros((5, n))
    data[0], data[4], data[2] = -1.0, -1.0, 4.0
    data[1] = np.where((j + 1) % m != 0, -1.0, 0.0)  # A[j + 1][j]
    data[3] = np.where(j % m != 0, -1.0, 0.0)  # A[j - 1][j]
    return offsets, data


@pytest.mark.parametrize("which", ["banded", "poisson"])
def test_converged_solve_against_csr_on_the_expansion(which):
    if which == "banded":
        n = 1000
        offsets, data = banded_dia(n)
        b = pp.system(n).b
    else:
        offsets, data = poisson_dia(48)
        n = 48 * 48
        b = np.random.default_rng(48).random(n) - 0.5
        A = do.dense(offsets, data, n)
        assert np.array_equal(A, A.T) and np.count_nonzero(A) == 5 * n - 4 * 48
    csr = do.expand(offsets, data, n)
    with from_dia(offsets, data) as sd, cg.Solver.from_csr(*csr) as sc:
        for s in (sd, sc):
            s.set_rows(0, b_rows=b, x_rows=np.zeros(n))
        xd, std = sd.solve(eps=1e-9)
        xc, stc = sc.solve(eps=1e-9)
    assert std.converged == 1 and stc.converged == 1
    assert rel(xd, xc) <= 1e-8, rel(xd, xc)
    no_hip_error()


# ---- 6. the preconditioner set-up's bits -------------------------------------------------------------------------------
def scrambled(n, seed=3):
    """banded_dia(n) with the diagonals unsorted and the main diagonal stored twice, in two pieces that sum to it only
    in the stored order; SPD as the original.  NaN in the unused slots."""
    offsets, data = banded_dia(n)
    by = {int(o): data[k] for k, o in enumerate(offsets)}
    a = np.random.default_rng([seed, n]).standard_normal(n)
    order = (37, 0, -1, 2, 0, 1, -37, -2)
    rows = []
    first = True
    for o in order:
        if o == 0:
            rows.append(by[0] + a if first else -a)
            first = False
        else:
            rows.append(by[o].copy())
    out = np.array(rows)
    for k, o in enumerate(order):
        lo, hi = do.in_range(o, n)
        out[k, :lo] = np.nan
        out[k, hi:] = np.nan
    return np.array(order, np.int32), out


def test_precond_setup_bits():
    n = 257
    offsets, data = scrambled(n)
    csr = do.expand(offsets, data, n)
    assert np.isfinite(csr[2]).all()
    with from_dia(offsets, data) as sd, cg.Solver.from_csr(*csr) as sc:
        sd.set_precond("jacobi")
        sc.set_precond("jacobi")
        assert same_bits(sd.precond_diag(), sc.precond_diag())
        assert not same_bits(sd.precond_diag(), 1.0 / pp.system(n).diag)  # the two pieces do round
        for pbs in range(2, 9):
            sd.set_precond_block(pbs)
            sc.set_precond_block(pbs)
            (gd, Wd), (gc, Wc) = sd.precond_block, sc.precond_block
            assert gd == gc == pbs and same_bits(Wd, Wc), pbs
    # no diagonal of offset 0: row 0 is named, the earlier preconditioner still gives its bits
    o2, d2 = banded_dia(n)
    keep = o2 != 0
    with from_dia(o2[keep], d2[keep], n=n) as sm:
        sm.set_precond_block(2, values=np.tile(np.eye(2), (-(-n // 2), 1, 1)))
        sm.set_rows(0, b_rows=pp.system(n).b, x_rows=np.zeros(n))
        x_before, _ = sm.solve(x0=np.zeros(n), eps=-1.0, max_iter=3)  # three fixed loops: the matrix is not SPD
        code, msg = code_of(lambda: sm.set_precond("jacobi"))
        assert code == ERR_SHAPE and "row 0 has no diagonal entry" in msg, msg
        assert sm.precond == "block"
        code, msg = code_of(lambda: sm.set_precond_block(3))
        assert code == ERR_SHAPE and sm.precond == "block" and sm.precond_block[0] == 2
        x_after, _ = sm.solve(x0=np.zeros(n), eps=-1.0, max_iter=3)
        assert same_bits(x_after, x_before)
    # a non-positive d_i: the lowest row is named
    d3 = d2.copy()
    d3[3, 5] = -1.0
    d3[3, 2] = 0.0
    with from_dia(o2, d3) as sm:
        sm.set_precond(np.full(n, 0.5))
        code, msg = code_of(lambda: sm.set_precond("jacobi"))
        assert code == ERR_SHAPE and "row 2 has the diagonal" in msg, msg
        assert sm.precond == "diag" and same_bits(sm.precond_diag(), np.full(n, 0.5))
    no_hip_error()


# ---- 7. the fused p.Ap -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,R,U", [(9, 1, 1), (60001, 1, 4), (60001, 2, 8), (18002, 2, 2)])
def test_fused_dot(n, R, U):
    """p.Ap of a context's diagonal matVec.  From x0 = 0 with b = +-1 the first loop has r.r = n exactly, p = b, and
    x_1 = alpha b with alpha = fl(n / p.Ap): p.Ap is read back as n / alpha, off by the division's one rounding,
    below 2^-52 |p.Ap|, which is added to the bar.  The reference is the exact (Fraction) dot of b with the emulated
    rows A b (b is +-1: the vectorised emulation is exact); the bar is the project's rule, 100 x the spread of
    three fp64 dots (floor 4 ulp), times sum |b_i| |(A b)_i|."""
    offsets = np.array([-2, 1, 0, -1, 2][:5 if n > 2 else 1], np.int32)
    data = np.random.default_rng(n).standard_normal((offsets.size, n))
    data[2] += 12.0  # a positive p.Ap is all the loop needs
    b = np.where(np.random.default_rng(n + 1).random(n) < 0.5, -1.0, 1.0)
    Ab = do.spmv_dia_pow2(offsets, data, b)
    if n == 9:
        assert same_bits(Ab, do.spmv_dia(offsets, data, b))
    ref = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(b, Ab))
    S = float(np.abs(Ab).sum())
    spread = max(abs(Fraction(float(dot(b, Ab))) - ref) / Fraction(S) for dot in pp.DOTS.values())
    bar = 100.0 * max(float(spread), pp.FLOOR)
    with from_dia(offsets, data) as s:
        s.set_matvec_plan(64 * R, U, 2)
        blocks = s.matvec_plan()["blocks"]
        assert (blocks == 1) == (n == 9)
        alphas = []
        for _ in range(2):
            s.set_rows(0, b_rows=b, x_rows=np.zeros(n))
            s.begin()
            assert s.iterate(1) == (1, False)
            x = s.get_x()
            alpha = x[0] * b[0]
            assert same_bits(x, alpha * b)
            alphas.append(alpha)
        assert alphas[0] == alphas[1]  # the same bits when run twice
        pap = Fraction(n) / Fraction(float(alphas[0]))
        err = float(abs(pap - ref))
        print(f"\n[dia fused dot] n={n} R={R} U={U} blocks={blocks}: |p.Ap - exact| / S = {err / S:.3g}, bar {bar:.3g}")
        assert err <= bar * S + 2.0 ** -52 * float(abs(ref))
    no_hip_error()


# ---- 8. lifecycle ------------------------------------------------------------------------------------------------------
def test_lifecycle_csr_dia_csr():
    n = 257
    sys_ = pp.system(n)
    csr, (offsets, data) = sys_.csr(), banded_dia(n)
    ndiag = offsets.size
    cap = ndiag * n
    with cg.Solver.from_csr(*csr) as fresh:
        fresh.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        xc, stc = fresh.solve(eps=1e-9)
        plan_c = fresh.matvec_plan()
    with cg.Solver(n, csr_nnz=cap) as s:
        s.set_csr(*csr)
        s.set_precond("jacobi")
        assert s.info.flags & cg.CGX_CSR_ACTIVE and not s.info.flags & DIA_ACTIVE
        s.set_dia(offsets, data)
        assert s.info.flags & DIA_ACTIVE and s.info.flags & cg.CGX_CSR_ACTIVE
        assert s.precond == "none" and not s.info.flags & cg.CGX_PRECOND_ACTIVE  # off after set_dia
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        xd, std = s.solve(eps=1e-9)
        assert std.converged == 1 and rel(xd, xc) <= 1e-8
        # plan refusals: the plan stays
        before = s.matvec_plan()
        for bad in ((32, 4, 2), (192, 4, 2), (64, 3, 2), (64, 16, 2), (64, 0, 2), (128, 4, 1), (128, 4, 0), (8, 1, 2)):
            code, msg = code_of(lambda: s.set_matvec_plan(*bad))
            assert code == ERR_ARG and s.matvec_plan() == before, (bad, msg)
        # a plan the caller chose on a diagonal-valued context survives the next set_dia
        s.set_matvec_plan(64, 2, 8)
        s.set_dia(offsets, data)
        pl = s.matvec_plan()
        assert (pl["R"], pl["U"], pl["nt"]) == (64, 2, 8)
        x_again, _ = s.solve(x0=np.zeros(n), eps=1e-9)
        assert rel(x_again, xd) <= 1e-8  # the rows' sums are the same bits; p.Ap's order follows the rows per wave
        xd, std = s.solve(x0=np.zeros(n), eps=1e-9)  # the bits under this plan, for the refusals below
        # failed cgx_set_dia calls, in the header's order: the earlier (diagonal) matrix still solves to the same bits
        L = cg.lib()
        o, d = np.ascontiguousarray(offsets), np.ascontiguousarray(data)
        po, pd = o.ctypes.data, d.ctypes.data
        err = lambda: L.cgx_last_error().decode()  # noqa: E731
        assert L.cgx_set_dia(None, ndiag, po, pd, n) == ERR_ARG and "ctx is NULL" in err()
        assert L.cgx_set_dia(s._h, -1, po, pd, n) == ERR_ARG and "ndiag" in err()
        assert L.cgx_set_dia(s._h, ndiag, None, pd, n) == ERR_ARG and "NULL" in err()
        assert L.cgx_set_dia(s._h, ndiag, po, None, n) == ERR_ARG and "NULL" in err()
        assert L.cgx_set_dia(s._h, ndiag, po, pd, n - 1) == ERR_SHAPE and "ld = 256" in err() and "n = 257" in err()
        more_o, more_d = np.concatenate([o, o[:1]]), np.concatenate([d, d[:1]])
        assert L.cgx_set_dia(s._h, ndiag + 1, more_o.ctypes.data, more_d.ctypes.data, n) == ERR_SHAPE
        assert "room for" in err() and str(cap) in err() and str((ndiag + 1) * n) in err()
        assert L.cgx_set_dia(s._h, 2 ** 62, po, pd, n) == ERR_SHAPE and "room for" in err()  # no overflow
        bad_o = o.copy()
        bad_o[4] = n
        assert L.cgx_set_dia(s._h, ndiag, bad_o.ctypes.data, pd, n) == ERR_SHAPE
        assert "cgx_dia_check" in err() and f"offsets[4] = {n}" in err()
        assert code_of(lambda: s.set_dia(bad_o, d))[0] == ERR_SHAPE
        assert s.info.flags & DIA_ACTIVE and s.matvec_plan() == pl
        xd2, std2 = s.solve(x0=np.zeros(n), eps=1e-9)
        assert same_bits(xd2, xd) and (std2.iterations, std2.rr) == (std.iterations, std.rr)
        # the zero matrix is a matrix
        s.set_dia(np.zeros(0, np.int32), np.zeros((0, n)))
        assert s.info.flags & DIA_ACTIVE
        assert L.cgx_set_dia(s._h, 0, None, None, n) == 0
        s.set_dia(offsets, data)
        # back to CSR: a fresh CSR context's bits
        s.set_csr(*csr)
        assert s.info.flags & cg.CGX_CSR_ACTIVE and not s.info.flags & DIA_ACTIVE
        assert s.matvec_plan() == plan_c
        x2, st2 = s.solve(x0=np.zeros(n), eps=1e-9)
        assert same_bits(x2, xc) and (st2.iterations, st2.rr) == (stc.iterations, stc.rr)
        # a failed set_dia on a scalar context leaves it scalar, solving to the same bits
        assert code_of(lambda: s.set_dia(bad_o, d))[0] == ERR_SHAPE
        assert not s.info.flags & DIA_ACTIVE
        x3, _ = s.solve(x0=np.zeros(n), eps=1e-9)
        assert same_bits(x3, xc)
    no_hip_error()


def test_lifecycle_bsr_dia_both_ways():
    bs, n = 3, 258
    sys_ = pp.system(n)
    bsr = bo.from_dense(sys_.dense(), bs)
    offsets, data = banded_dia(n)
    cap = max(int(bsr[1].size) * bs * bs, offsets.size * n)
    with cg.Solver.from_bsr(*bsr) as fresh:
        fresh.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        xb, stb = fresh.solve(eps=1e-9)
        plan_b = fresh.matvec_plan()
    with from_dia(offsets, data) as fresh:
        fresh.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        xd, std = fresh.solve(eps=1e-9)
        plan_d = fresh.matvec_plan()
    with cg.Solver(n, csr_nnz=cap) as s:
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        for _ in range(2):
            s.set_bsr(*bsr)
            f = s.info.flags
            assert f & cg.CGX_BSR_ACTIVE and f & cg.CGX_CSR_ACTIVE and not f & DIA_ACTIVE
            assert s.matvec_plan() == plan_b
            x, st = s.solve(x0=np.zeros(n), eps=1e-9)
            assert same_bits(x, xb) and (st.iterations, st.rr) == (stb.iterations, stb.rr)
            s.set_dia(offsets, data)
            f = s.info.flags
            assert f & DIA_ACTIVE and f & cg.CGX_CSR_ACTIVE and not f & cg.CGX_BSR_ACTIVE
            assert s.matvec_plan() == plan_d
            x, st = s.solve(x0=np.zeros(n), eps=1e-9)
            assert same_bits(x, xd) and (st.iterations, st.rr) == (std.iterations, std.rr)
    no_hip_error()


def test_set_dia_refused_on_other_contexts():
    offsets, data = banded_dia(258)
    o, d = np.ascontiguousarray(offsets), np.ascontiguousarray(data)
    L = cg.lib()
    args = (o.size, o.ctypes.data, d.ctypes.data, 258)
    nnz = o.size * 258
    with cg.Solver.csr(258, nnz, nrhs=2) as s:
        assert L.cgx_set_dia(s._h, *args) == ERR_ARG
        assert "right-hand sides" in L.cgx_last_error().decode() and "not built" in L.cgx_last_error().decode()
        with pytest.raises(ValueError):
            s.set_dia(offsets, data)
    with cg.Solver.csr(258, nnz, devices=[0, 0]) as s:
        assert L.cgx_set_dia(s._h, *args) == ERR_ARG
        assert "row blocks" in L.cgx_last_error().decode() and "not built" in L.cgx_last_error().decode()
    with cg.Solver.csr(258, nnz, devices=[0]) as s:
        assert L.cgx_set_dia(s._h, *args) == ERR_ARG
    with cg.Solver(258) as s:
        assert L.cgx_set_dia(s._h, *args) == ERR_ARG and "not a cgx_create_csr context" in L.cgx_last_error().decode()
    with cg.Solver(None, poisson_m=16) as s:
        assert L.cgx_set_dia(s._h, *args) == ERR_ARG
    no_hip_error()


def test_odd_n_at_full_capacity_takes_the_library_buffer():
    """n odd and ndiag n == the capacity: the even pitch does not fit the context's values, so the diagonals go to the
    library's own memory; the bits are those of a roomier context."""
    n = 257
    sys_ = pp.system(n)
    offsets, data = banded_dia(n)
    out = []
    for cap in (offsets.size * n, offsets.size * (n + 1)):
        with cg.Solver(n, csr_nnz=cap) as s:
            s.set_dia(offsets, data)
            s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
            out.append(s.solve(eps=1e-9)[0])
    assert same_bits(*out)
    no_hip_error()


# ---- 9. CLI ------------------------------------------------------------------------------------------------------------
def test_cli_dia(tmp_path):
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

    def run(*opts):
        r = subprocess.run([cg.CLI_PATH, *opts, "--eps", "1e-12", "--print-x", "--stats", *paths],
                           capture_output=True, text=True, timeout=300, env=one_gpu)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().splitlines()
        return lines[:-n], np.array([float(v) for v in lines[-n:]])

    head_c, x_c = run("--csr")
    head_d, x_d = run("--csr", "--dia")
    assert head_d[0] == head_c[0] == f"Computing cg of matrix size : {n * n}"
    assert head_d[2].startswith("iterations: ") and " converged: 1 " in head_d[2], head_d[2]
    assert head_d[2].split(" residual_norm")[0] == head_c[2].split(" residual_norm")[0]  # the same converged line
    assert head_d[3] == head_c[3] == f"nnz: {np.count_nonzero(Aw)}"
    assert head_d[4] == f"ndiag: {do.from_dense(Aw)[0].size}" == "ndiag: 7" and len(head_d) == len(head_c) + 1
    assert rel(x_d, x_c) <= 1e-8
    assert np.linalg.norm(bw - Aw @ x_d) <= 1e-10 * np.linalg.norm(bw)
    head_j, x_j = run("--csr", "--dia", "--jacobi")
    assert head_j[4] == "ndiag: 7" and head_j[5] == "precond: jacobi" and " converged: 1 " in head_j[2]
    assert rel(x_j, x_c) <= 1e-8
    head_b, x_b = run("--csr", "--dia", "--block-jacobi", "4")
    assert head_b[5] == "precond: block-jacobi 4" and " converged: 1 " in head_b[2] and rel(x_b, x_c) <= 1e-8
    for opts in (("--dia",), ("--csr-a32", "--dia"), ("--csr", "--dia", "--bsr", "2")):
        r = subprocess.run([cg.CLI_PATH, *opts, *paths], capture_output=True, text=True, timeout=60, env=one_gpu)
        assert r.returncode != 0 and "--dia holds a --csr matrix by its diagonals" in r.stderr, (opts, r.stderr)
