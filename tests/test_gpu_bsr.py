"""cgx_set_bsr: a block-valued cgx_create_csr context (k_bsr_mult_f64, csrc/cgx_bsmv.hip) through every layer.

  1. the kernel's bits against the CPU statement of its summation order (tests/_bsmv_order.py) at every block size,
     T and load policy, kernel-level and through a context;
  2. the grid-stride walk under one block per CU;
  3. the element-wise probe of the iteration, plain and under every preconditioner kind, against the long-double
     references and bars of tests/_nrhs_probe.py and tests/_pcg_probe.py (tests/test_bsmv_order_cpu.py asserts those
     bars at these sizes);
  4. the host forms; 5. converged solves against the oracle; 6. the preconditioner set-up's bits against a CSR
     context on the expanded matrix; 7. the fused p.Ap; 8. the lifecycle and the refusals; 9. `cg_hip --csr --bsr`.

The probe's matrix is ``_pcg_probe.system(n)`` held as BSR: every bs x bs block that holds an entry, zero-filled
(tests/_bsmv_order.from_dense), at n = the smallest multiples of bs >= 257 and >= 2049."""
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _bsmv_order as bo
import _nrhs_probe as npr
import _pcg_probe as pp
import conjugate_gradient_amd as cg
import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-10
ERR_ARG, ERR_SHAPE = -1, -4
LD = np.longdouble
# None on a tree without the feature: every test then fails at its first use
spmv_bsr = getattr(cg, "spmv_bsr", None)
from_bsr = getattr(cg.Solver, "from_bsr", None)
BSR_ACTIVE = getattr(cg, "CGX_BSR_ACTIVE", None)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert hasattr(cg.Solver, "set_bsr"), "the package has no block storage"


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


def probe_sizes(bs):
    return tuple(-(-m // bs) * bs for m in (257, 2049))


@functools.lru_cache(maxsize=None)
def banded_bsr(n, bs):
    """_pcg_probe.system(n) as BSR, blocks zero-filled; read-only."""
    out = bo.from_dense(pp.system(n).dense(), bs)
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. order ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def struct(bs):
    return bo.structure_matrix(bs)


@functools.lru_cache(maxsize=None)
def struct_expected(bs, T):
    return bo.spmv_bsr(*struct(bs), T)


def run_kernel(indptr, indices, data, v, nb, ncolb, spare=3):
    bs = data.shape[1]
    dv = cg.DeviceArray.from_host(v)
    dout = cg.DeviceArray.from_host(np.full(nb * bs + spare, np.nan))
    spmv_bsr(indptr, indices, data, dv, dout, nb, ncolb)
    out = dout.to_host()
    dv.free()
    dout.free()
    assert np.isnan(out[nb * bs:]).all(), "the kernel stored past the last row"
    return out[:nb * bs]


@pytest.mark.parametrize("nt", bo.POLICIES)
@pytest.mark.parametrize("T", bo.TS)
@pytest.mark.parametrize("bs", bo.BLOCK_SIZES)
def test_structure_matrix_bits(monkeypatch, bs, T, nt):
    indptr, indices, data, v = struct(bs)
    monkeypatch.setenv("CGX_BSMV_PLAN", f"T={T},nt={nt}")
    out = run_kernel(indptr, indices, data, v, bo.STRUCT_NB, bo.STRUCT_NCOLB)
    want = struct_expected(bs, T)
    assert same_bits(out, want), (bs, T, nt, np.flatnonzero(out != want))
    no_hip_error()


def test_plan_string_naming_no_plan_runs_the_default(monkeypatch):
    indptr, indices, data, v = struct(3)
    monkeypatch.delenv("CGX_BSMV_PLAN", raising=False)
    default = run_kernel(indptr, indices, data, v, bo.STRUCT_NB, bo.STRUCT_NCOLB)
    assert same_bits(default, struct_expected(3, 8))  # the kernel-level call's default T
    for plan in ("T=3,nt=2", "T=8,nt=1", "T=128,nt=8", "T=0"):
        monkeypatch.setenv("CGX_BSMV_PLAN", plan)
        assert same_bits(run_kernel(indptr, indices, data, v, bo.STRUCT_NB, bo.STRUCT_NCOLB), default)


def test_python_never_launches_on_unchecked_indices():
    indptr, indices, data, v = struct(2)
    dv, dout = cg.DeviceArray.from_host(v), cg.DeviceArray.from_host(np.full(50, np.nan))
    for bad in (bo.STRUCT_NCOLB, -1):
        idx = indices.copy()
        idx[17] = bad
        with pytest.raises((cg.CgxError, ValueError)):
            spmv_bsr(indptr, idx, data, dv, dout, bo.STRUCT_NB, bo.STRUCT_NCOLB)
    assert np.isnan(dout.to_host()).all()  # nothing ran


@functools.lru_cache(maxsize=None)
def square_struct(bs):
    """The structure matrix's block rows with block columns inside [0, STRUCT_NB): a context's matrix is square."""
    indptr, indices, data, v = bo.structure_matrix(bs, seed=20262)
    return indptr, (indices % bo.STRUCT_NB).astype(np.int32), data, v[:bo.STRUCT_NB * bs].copy()


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("bs", bo.BLOCK_SIZES)
def test_structure_matrix_bits_through_a_context(bs):
    """A context's matVec, read back through one fixed loop from x0 = v with b = 0: r_0 = 0 - A v exactly, p_0 = r_0,
    and x_1[i] = fma(alpha, p_0[i], v[i]) with the one alpha of the loop.  With w = the emulation's A v, some double
    alpha within a few ulp of (v[i] - x_1[i]) / w[i] must give every element of x_1 bit for bit; a w that differs
    from the kernel's in one bit of one row has none.  (The matrix need not be SPD for one fixed loop.)"""
    indptr, indices, data, v = square_struct(bs)
    n = bo.STRUCT_NB * bs
    live = np.repeat(np.diff(indptr) > 0, bs)
    with from_bsr(indptr, indices, data) as s:
        assert s.info.flags & BSR_ACTIVE and s.info.flags & cg.CGX_CSR_ACTIVE
        for T in bo.TS:
            w = bo.spmv_bsr(indptr, indices, data, v, T)
            for nt in bo.POLICIES:
                s.set_matvec_plan(64 // T, 1, nt)
                pl = s.matvec_plan()
                assert (pl["R"], pl["U"], pl["nt"]) == (64 // T, 1, nt)
                s.set_rows(0, b_rows=np.zeros(n), x_rows=v)
                s.begin()
                assert s.iterate(1) == (1, False)
                x1 = s.get_x()
                assert same_bits(x1[~live], v[~live])  # an empty block row: p = -(+0.0), x unchanged
                # the row where alpha w weighs most against x: the least cancellation in v - x_1
                i0 = int(np.argmax(np.abs(w) / np.maximum(np.abs(v), np.abs(x1))))
                guess = (v[i0] - x1[i0]) / w[i0]
                cands = [guess]
                for _ in range(64):
                    cands = [np.nextafter(cands[0], -np.inf)] + cands + [np.nextafter(cands[-1], np.inf)]
                rows = np.flatnonzero(live)
                hit = [a for a in cands if all(fma(a, -w[i], v[i]) == x1[i] for i in rows)]
                assert hit, (bs, T, nt)
    no_hip_error()


# ---- 2. the grid-stride walk -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 64])
@pytest.mark.parametrize("bs", [2, 3, 8])
def test_grid_stride_walk(monkeypatch, bs, T):
    """100,001 block rows under one block per CU: on 256 CUs a sweep covers 1024 waves x 64 / T block rows (32,768 /
    1,024), so a wave walks several groups and the last group is partial."""
    nb = 100001
    v = bo.pow2_vector(nb * bs)
    monkeypatch.setenv("CGX_BSMV_PLAN", f"T={T},nt=2,bpc=1")
    out = run_kernel(*bo.block_tridiag(nb, bs), v, nb, nb)
    want = bo.spmv_block_tridiag(nb, bs, v, T)
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
    print(f"\n[bsr probe] {what}: " + ", ".join(f"k={k} {v:.3g} of the bar" for k, v in worst.items()))
    assert not bad, (what, bad)
    s.set_rows(0, x_rows=x0)
    again = snapshots(s)
    assert all(same_bits(a[0], x[0]) and a[1] == x[1] for a, x in zip(again, snaps))
    x3, st = s.solve(x0=x0, eps=-1.0, max_iter=max(pp.KS))
    assert st.iterations == max(pp.KS) and same_bits(x3, snaps[-1][0])


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("bs", bo.BLOCK_SIZES)
def test_iteration_probe(bs, big):
    n = probe_sizes(bs)[big]
    assert n % bs == 0 and n - bs < (2049 if big else 257) <= n
    sys_ = pp.system(n)
    with from_bsr(*banded_bsr(n, bs)) as s:
        assert s.info.flags & BSR_ACTIVE
        for zero in (False, True):
            tag = f"bs {bs} n {n} x0 {'0' if zero else 'rough'}"
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
            for kind, pbs in (("jacobi", 0), ("diag", 0), ("block", bs)):
                case = pp.Case(kind, pbs, n, zero)
                if kind == "block":
                    s.set_precond_block(bs, values=pp.blocks(n, bs)[1])
                else:
                    s.set_precond(pp.library_precond(case))
                assert s.precond == kind
                if kind == "jacobi":  # extracted from the BSR arrays: 1 / diag(A) bit for bit
                    assert same_bits(s.precond_diag(), 1.0 / sys_.diag)
                pr = pp.probe(case)
                run_probe(s, sys_.b, x0, {k: (pr.X[k], pr.S[k], pp.bar(case, k)) for k in pp.KS}, f"{kind} " + tag)
    no_hip_error()


# ---- 4. host forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [3, 4])
def test_host_forms(monkeypatch, bs):
    n = probe_sizes(bs)[1]
    sys_ = pp.system(n)
    eps = 1e-9
    monkeypatch.delenv("CGX_GATED", raising=False)
    with from_bsr(*banded_bsr(n, bs)) as s:
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
        rn, bn = s.residual_norm()  # the block kernel again
        A = sys_.dense()
        assert abs(rn - np.linalg.norm(sys_.b - A @ x1)) <= 1e-12 * np.linalg.norm(sys_.b)
        assert abs(bn - np.linalg.norm(sys_.b)) <= 1e-12 * np.linalg.norm(sys_.b)
    no_hip_error()


# ---- 5. converged solves -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_solution(n):
    sys_ = pp.system(n)
    xo, st = oracle.cg_f64(sys_.dense(), sys_.b, np.zeros(n), eps=1e-12)
    assert st.converged == 1
    xo.setflags(write=False)
    return xo


@pytest.mark.parametrize("precond", [None, "block"])
@pytest.mark.parametrize("bs", [2, 3, 5, 8])
def test_converged_solve(bs, precond):
    n = -(-1000 // bs) * bs
    sys_ = pp.system(n)
    xo = oracle_solution(n)
    with from_bsr(*banded_bsr(n, bs), precond=("block", bs) if precond else None) as s:
        assert s.precond == (precond or "none")
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        x, st = s.solve(eps=1e-12)
    assert st.converged == 1
    A = sys_.dense()
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(sys_.b - A @ x) <= TOL * np.linalg.norm(sys_.b)
    no_hip_error()


# ---- 6. the preconditioner set-up's bits -------------------------------------------------------------------------------
def scrambled(n, bs, seed=3):
    """banded_bsr(n, bs) with every block row's blocks shuffled and every diagonal block stored in three pieces that
    sum to it only in the stored order; SPD as the original."""
    indptr, indices, data = banded_bsr(n, bs)
    rng = np.random.default_rng([seed, n, bs])
    rp, ci, va = [0], [], []
    for I in range(n // bs):
        cols, blks = [], []
        for q in range(indptr[I], indptr[I + 1]):
            if indices[q] == I:
                a, b = rng.standard_normal((2, bs, bs))
                pieces = [data[q] + a, -a + b, -b]
            else:
                pieces = [data[q]]
            cols += [int(indices[q])] * len(pieces)
            blks += pieces
        order = rng.permutation(len(cols))
        ci += [cols[o] for o in order]
        va += [blks[o] for o in order]
        rp.append(len(ci))
    return np.array(rp, np.int64), np.array(ci, np.int32), np.array(va)


@pytest.mark.parametrize("bs", [2, 3, 5, 8])
def test_precond_setup_bits(bs):
    n = probe_sizes(bs)[0]
    bsr = scrambled(n, bs)
    first = bsr[1][:bsr[0][1]]
    assert np.count_nonzero(first == 0) == 3 and np.any(np.diff(first) < 0)  # a diagonal block in pieces, unsorted
    csr = bo.expand(*bsr)
    with from_bsr(*bsr) as sb, cg.Solver.from_csr(*csr) as sc:
        sb.set_precond("jacobi")
        sc.set_precond("jacobi")
        assert same_bits(sb.precond_diag(), sc.precond_diag())
        for pbs in (2, 3, 8):
            sb.set_precond_block(pbs)
            sc.set_precond_block(pbs)
            (gb, Wb), (gc, Wc) = sb.precond_block, sc.precond_block
            assert gb == gc == pbs and same_bits(Wb, Wc), (bs, pbs)
        # a missing diagonal block: the lowest row is named, the earlier preconditioner still gives its bits
        rp, ci, va = (a.copy() for a in bsr)
        drop = [q for I in (5, 2) for q in range(rp[I], rp[I + 1]) if ci[q] == I]
        keep = np.setdiff1d(np.arange(ci.size), drop)
        rp2 = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n // bs), np.diff(rp))[keep],
                                                         minlength=n // bs))]).astype(np.int64)
        with from_bsr(rp2, ci[keep], va[keep]) as sm:
            sm.set_precond_block(2, values=np.tile(np.eye(2), (-(-n // 2), 1, 1)))
            sm.set_rows(0, b_rows=pp.system(n).b, x_rows=np.zeros(n))
            x_before, _ = sm.solve(x0=np.zeros(n), eps=-1.0, max_iter=3)  # three fixed loops: the matrix is not SPD
            code, msg = code_of(lambda: sm.set_precond("jacobi"))
            assert code == ERR_SHAPE and f"row {2 * bs} has no diagonal entry" in msg, msg
            assert sm.precond == "block"
            code, msg = code_of(lambda: sm.set_precond_block(bs))
            assert code == ERR_SHAPE and sm.precond == "block" and sm.precond_block[0] == 2
            x_after, _ = sm.solve(x0=np.zeros(n), eps=-1.0, max_iter=3)
            assert same_bits(x_after, x_before)
    no_hip_error()


# ---- 7. the fused p.Ap -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,bs,T", [(9, 3, 8), (20001, 3, 2), (6001, 8, 4)])
def test_fused_dot(monkeypatch, nb, bs, T):
    """p.Ap of a context's block matVec.  From x0 = 0 with b = +-1 the first loop has r.r = n exactly, p = b, and
    x_1 = alpha b with alpha = fl(n / p.Ap): p.Ap is read back as n / alpha, off by the division's one rounding,
    below 2^-52 |p.Ap|, which is added to the bar (it is under 1 % of the bar's floor).  The reference is the long-double dot of b with the kernel's
    own A b (the kernel-level call at the same T: a row's sum depends on (bs, T) only); the bar is the project's rule,
    100 x the spread of three fp64 dots (floor 4 ulp), times sum |b_i| |(A b)_i|."""
    n = nb * bs
    indptr, indices, data = bo.block_tridiag(nb, bs)
    data = data.copy()
    d = np.flatnonzero(indices == np.repeat(np.arange(nb), np.diff(indptr)))
    data[d] += 4.0 * bs * np.eye(bs)  # a positive p.Ap is all the loop needs
    b = np.where(np.random.default_rng(nb).random(n) < 0.5, -1.0, 1.0)
    monkeypatch.setenv("CGX_BSMV_PLAN", f"T={T},nt=2")
    Ab = run_kernel(indptr, indices, data, b, nb, nb)
    monkeypatch.delenv("CGX_BSMV_PLAN")
    ref = np.dot(b.astype(LD), Ab.astype(LD))
    S = float(np.abs(Ab).sum())
    spread = max(abs(LD(dot(b, Ab)) - ref) / S for dot in pp.DOTS.values())
    bar = 100.0 * max(float(spread), pp.FLOOR)
    with from_bsr(indptr, indices, data) as s:
        s.set_matvec_plan(64 // T, 1, 2)
        blocks = s.matvec_plan()["blocks"]
        assert (blocks == 1) == (nb == 9)
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
        pap = LD(n) / LD(alphas[0])
        err = float(abs(pap - ref))
        print(f"\n[bsr fused dot] nb={nb} bs={bs} T={T} blocks={blocks}: |p.Ap - ld| / S = {err / S:.3g}, bar {bar:.3g}")
        assert err <= bar * S + 2.0 ** -52 * float(abs(ref))
    no_hip_error()


# ---- 8. lifecycle ------------------------------------------------------------------------------------------------------
def test_lifecycle_csr_bsr_csr():
    bs, n = 3, probe_sizes(3)[0]
    sys_ = pp.system(n)
    csr, bsr = sys_.csr(), banded_bsr(n, bs)
    cap = int(bsr[1].size) * bs * bs
    with cg.Solver.from_csr(*csr) as fresh:
        fresh.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        xc, stc = fresh.solve(eps=1e-9)
        plan_c = fresh.matvec_plan()
    with cg.Solver(n, csr_nnz=cap) as s:
        s.set_csr(*csr)
        s.set_precond("jacobi")
        assert s.info.flags & cg.CGX_CSR_ACTIVE and not s.info.flags & BSR_ACTIVE
        s.set_bsr(*bsr)
        assert s.info.flags & BSR_ACTIVE and s.info.flags & cg.CGX_CSR_ACTIVE
        assert s.precond == "none" and not s.info.flags & cg.CGX_PRECOND_ACTIVE  # off after set_bsr
        s.set_rows(0, b_rows=sys_.b, x_rows=np.zeros(n))
        xb, stb = s.solve(eps=1e-9)
        assert stb.converged == 1 and rel(xb, xc) <= 1e-8
        # plan refusals as on CSR: the plan stays
        before = s.matvec_plan()
        for bad in ((3, 1, 2), (64, 1, 2), (8, 2, 2), (8, 1, 1), (8, 1, 0)):
            code, msg = code_of(lambda: s.set_matvec_plan(*bad))
            assert code == ERR_ARG and s.matvec_plan() == before, (bad, msg)
        # failed set_bsr calls: the earlier (block) matrix still solves to the same bits
        idx = bsr[1].copy()
        idx[len(idx) // 2] = n // bs
        assert code_of(lambda: s.set_bsr(bsr[0], idx, bsr[2]))[0] == ERR_SHAPE
        assert "bcol_idx" in code_of(lambda: s.set_bsr(bsr[0], idx, bsr[2]))[1]
        L = cg.lib()
        rp, ci, va = (np.ascontiguousarray(a) for a in bsr)
        big_rp = np.concatenate([rp, [rp[-1]]])  # the C call itself: the mirror refuses these before it
        more = np.concatenate([ci, ci[:1]]), np.concatenate([va, va[:1]])
        over_rp = rp.copy()
        over_rp[-1] += 1
        assert L.cgx_set_bsr(s._h, bs, over_rp.ctypes.data, more[0].ctypes.data, more[1].ctypes.data) == ERR_SHAPE
        assert "room for" in L.cgx_last_error().decode()
        assert n % 4 != 0
        assert L.cgx_set_bsr(s._h, 4, big_rp.ctypes.data, ci.ctypes.data, va.ctypes.data) == ERR_SHAPE  # n % bs
        assert "not divisible" in L.cgx_last_error().decode()
        for b1 in (1, 9, 0, -3):
            assert L.cgx_set_bsr(s._h, b1, rp.ctypes.data, ci.ctypes.data, va.ctypes.data) == ERR_ARG
        assert L.cgx_set_bsr(s._h, bs, None, ci.ctypes.data, va.ctypes.data) == ERR_ARG
        assert L.cgx_set_bsr(s._h, bs, rp.ctypes.data, None, va.ctypes.data) == ERR_ARG
        assert L.cgx_set_bsr(s._h, bs, rp.ctypes.data, ci.ctypes.data, None) == ERR_ARG
        assert s.info.flags & BSR_ACTIVE
        xb2, stb2 = s.solve(x0=np.zeros(n), eps=1e-9)
        assert same_bits(xb2, xb) and (stb2.iterations, stb2.rr) == (stb.iterations, stb.rr)
        # back to CSR: a fresh CSR context's bits
        s.set_csr(*csr)
        assert s.info.flags & cg.CGX_CSR_ACTIVE and not s.info.flags & BSR_ACTIVE
        assert s.matvec_plan() == plan_c
        x2, st2 = s.solve(x0=np.zeros(n), eps=1e-9)
        assert same_bits(x2, xc) and (st2.iterations, st2.rr) == (stc.iterations, stc.rr)
        # a failed set_bsr on a scalar context leaves it scalar, solving to the same bits
        assert code_of(lambda: s.set_bsr(bsr[0], idx, bsr[2]))[0] == ERR_SHAPE
        assert not s.info.flags & BSR_ACTIVE
        x3, _ = s.solve(x0=np.zeros(n), eps=1e-9)
        assert same_bits(x3, xc)
    no_hip_error()


def test_set_bsr_refused_on_other_contexts():
    rp, ci, va = banded_bsr(258, 2)
    L = cg.lib()
    args = (2, rp.ctypes.data, ci.ctypes.data, va.ctypes.data)
    nnz = int(ci.size) * 4
    with cg.Solver.csr(258, nnz, nrhs=2) as s:
        assert L.cgx_set_bsr(s._h, *args) == ERR_ARG and "right-hand sides" in L.cgx_last_error().decode()
    with cg.Solver.csr(258, nnz, devices=[0, 0]) as s:
        assert L.cgx_set_bsr(s._h, *args) == ERR_ARG and "row blocks" in L.cgx_last_error().decode()
    with cg.Solver.csr(258, nnz, devices=[0]) as s:
        assert L.cgx_set_bsr(s._h, *args) == ERR_ARG
    with cg.Solver(258) as s:
        assert L.cgx_set_bsr(s._h, *args) == ERR_ARG and "not a cgx_create_csr context" in L.cgx_last_error().decode()
    with cg.Solver(None, poisson_m=16) as s:
        assert L.cgx_set_bsr(s._h, *args) == ERR_ARG
    no_hip_error()


# ---- 9. CLI ------------------------------------------------------------------------------------------------------------
ONE_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="0")


def test_cli_bsr_block_jacobi(tmp_path):
    n = 130
    sys_ = pp.system(n)
    for name, arr, dec in (("A.txt", sys_.dense(), 6), ("b.txt", sys_.b, 9), ("x0.txt", np.zeros(n), 1)):
        oracle.write_text(str(tmp_path / name), arr, dec)
    paths = [str(tmp_path / f) for f in ("A.txt", "b.txt", "x0.txt")]
    Aw = cg.read_text(paths[0], n * n, np.float64).reshape(n, n)  # the matrix as the file holds it
    bw = cg.read_text(paths[1], n, np.float64)
    xo, st = oracle.cg_f64(Aw, bw, np.zeros(n), eps=1e-12)
    assert st.converged == 1
    r = subprocess.run([cg.CLI_PATH, "--csr", "--bsr", "5", "--block-jacobi", "5", "--eps", "1e-12", "--print-x",
                        "--stats", *paths], capture_output=True, text=True, timeout=300, env=ONE_GPU)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"Computing cg of matrix size : {n * n}"
    assert lines[2].startswith("iterations: ") and " converged: 1 " in lines[2], lines[2]
    assert lines[3] == f"nnz: {np.count_nonzero(Aw)}"
    assert lines[4] == f"nnzb: {bo.from_dense(Aw, 5)[1].size}"
    assert lines[5] == "precond: block-jacobi 5"
    x = np.array([float(v) for v in lines[-n:]])
    assert len(lines) == 6 + n and rel(x, xo) <= TOL
    assert np.linalg.norm(bw - Aw @ x) <= TOL * np.linalg.norm(bw)
