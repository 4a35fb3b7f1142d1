"""cgx_create_csr_multi: a sparse A over equal row blocks in one process, with the indexed exchange of p
(k_gather_indexed) -- the kernel alone, one block against cgx_create_csr, every partition against the oracle, every
exchange and host form to the same bits, the element-wise probe of tests/_nrhs_probe.py, replacing the matrix, the
lifecycle and the refusals.  Every block runs on device 0 except in the last test.

Systems.  Masked: tests/test_gpu_csr_nrhs.py's (its docstring holds the oracle's measured margins: (1000, 2) column 0
stops after 6 loops at 5.96 / 0.203 of the threshold, (2100, 8) after 6 at 8.95 / 0.024; Poisson m = 12, b = 1 after
21 at 362 / 2.4e-6).  Banded: tests/_pcg_probe.py's system (diagonal 4 + u, bands at 1, 2 and 37) with
tests/_nrhs_probe.py's column 0 as b and x0.

The bar of a converged solve is the project's fp64 one: the oracle's loop count, ||x - x_oracle|| <= 1e-10
||x_oracle||, ||b - A x|| <= max(1e-10 ||b||, 1e-10).  The probe's bars are tests/_nrhs_probe.py's own (100 x the
measured spread between fp64 summation orders, floored at 4 ulp): the block-order combine of the partial sums is one
more summation order.  Float-stored values are probed against the same recurrence in long double on the widened
matrix, with bars measured on that matrix by the same rule."""
import functools

import numpy as np
import pytest

import _csr_multi as cm
import _nrhs_probe as nq
import conjugate_gradient_amd as cg
import oracle
from test_gpu_csr_nrhs import column, masked

pytestmark = pytest.mark.gpu
TOL = 1e-10
EPS = 1e-10
# None on a tree without the feature: every test then fails at its first use
HALO_ACTIVE = getattr(cg, "CGX_CSR_HALO_ACTIVE", None)
gather_indexed = getattr(cg, "gather_indexed", None)
halo_counts = getattr(cg, "csr_halo_counts", None)
ENV = ("CGX_CSR_XCHG", "CGX_LOCAL_XCHG", "CGX_LOCAL_FUSE", "CGX_LOCAL_THREADS", "CGX_GATED", "CGX_SPMV_PLAN")


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert HALO_ACTIVE is not None, "the package has no CSR contexts over row blocks"


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def no_hip_error():
    assert cg.lib().cgx_hip_last_error() == 0


def blocks(csr, b, P, x0=None, devices=None, **kw):
    """A context over P row blocks (on device 0 unless `devices`) with the matrix, b and x0 (0) set."""
    s = cg.Solver.from_csr(*csr, devices=devices or [0] * P, **kw)
    try:
        s.set_rows(0, b_rows=b, x_rows=np.zeros(b.size) if x0 is None else x0)
    except Exception:
        s.close()
        raise
    return s


def meets_bar(x, st, A, b, xo, K):
    assert (st.iterations, st.converged) == (K, 1), (st.iterations, st.converged, K)
    assert rel(x, xo) <= TOL, rel(x, xo)
    assert np.linalg.norm(b - A @ x) <= max(TOL * np.linalg.norm(b), EPS)


@functools.lru_cache(maxsize=None)
def banded(n):
    """(csr, A dense, b, rough x0) of the banded system of n rows."""
    op = nq.operator("csr", n)
    b, x0 = nq.column_data(n, 0)
    return op.csr(), op.dense(), b, x0


# ---- 1. the kernel alone ------------------------------------------------------------------------------------
# one pass of the capped grid moves 64 blocks x 256 threads x 8 entries = 131072
@pytest.mark.parametrize("count", [0, 1, 2, 2047, 2048, 2049, 131071, 131072, 131073])
def test_gather_indexed_alone(count):
    rng = np.random.default_rng([count, 17])
    n = 2 * count + 7
    src = rng.standard_normal(n)
    idx = np.sort(rng.choice(n, size=count, replace=False)).astype(np.int32)
    want = np.full(n, np.nan)
    want[idx] = src[idx]
    d_src, d_idx = cg.DeviceArray.from_host(src), cg.DeviceArray.from_host(idx)
    d_dst = cg.DeviceArray.from_host(np.full(n, np.nan))
    try:
        gather_indexed(d_src, d_idx, d_dst)
        got = d_dst.to_host()
    finally:
        for d in (d_src, d_idx, d_dst):
            d.free()
    assert same_bits(got, want)  # the listed entries, and NaN everywhere else
    assert np.count_nonzero(~np.isnan(got)) == count
    no_hip_error()
    if count == 2049:  # the Python mirror refuses an index outside either array before the launch
        arrs = (cg.DeviceArray(n), cg.DeviceArray.from_host(np.array([0, n], np.int32)), cg.DeviceArray(n))
        try:
            with pytest.raises(ValueError, match="outside"):
                gather_indexed(*arrs)
        finally:
            for d in arrs:
                d.free()


# ---- 2. one block is cgx_create_csr -----------------------------------------------------------------------------
@pytest.mark.parametrize("a_f32", [False, True])
def test_one_block_is_create_csr(a_f32):
    csr = masked(1000, 2)[1]
    b = column(1000, 2, 0, 1.0)[0]
    with cg.Solver.from_csr(*csr, a_f32=a_f32) as one, blocks(csr, b, 1, a_f32=a_f32) as s:
        one.set_rows(0, b_rows=b, x_rows=np.zeros(1000))
        info = s.info
        assert info.nshards == 1 and info.flags & cg.CGX_CSR_ACTIVE and not info.flags & HALO_ACTIVE
        assert bool(info.flags & cg.CGX_A_F32) == a_f32
        assert s.csr_halo().tolist() == [[0]]
        for plan in (None, (8, 1, 8), (2, 1, 2)):
            if plan:
                one.set_matvec_plan(*plan)
                s.set_matvec_plan(*plan)
            assert s.matvec_plan() == one.matvec_plan()
            x1, st1 = one.solve(x0=np.zeros(1000), eps=EPS)
            x, st = s.solve(x0=np.zeros(1000), eps=EPS)
            assert st1.converged == 1 and (st.iterations, st.converged) == (st1.iterations, 1)
            assert same_bits(x, x1) and same_bits(st.rr, st1.rr), plan
    no_hip_error()


# ---- 3. parity per partition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,P", [(1000, 2, 2), (1000, 2, 4), (1000, 2, 8), (2100, 8, 3), (2100, 8, 4)])
def test_parity_per_partition(n, seed, P):
    A, csr = masked(n, seed)
    b, xo, K = column(n, seed, 0, 1.0)  # checked_oracle: the factor-3 margin asserted on the oracle alone
    assert K == 6
    with blocks(csr, b, P) as s:
        assert s.info.flags & HALO_ACTIVE and s.info.nshards == P
        assert np.array_equal(s.csr_halo(), cm.expected_counts(csr[0], csr[1], P))
        x, st = s.solve(eps=EPS)
        meets_bar(x, st, A, b, xo, K)
    no_hip_error()


@pytest.mark.parametrize("P", [2, 3, 4, 6])
def test_parity_poisson(P):
    m, n = 12, 144
    b = np.ones(n)
    xo, so = oracle.cg_poisson_f64(m, b, np.zeros(n), eps=EPS)
    K = so.iterations
    before = np.sqrt(oracle.cg_poisson_f64(m, b, np.zeros(n), max_iter=K - 1, eps=-1.0)[1].rr) / EPS
    assert so.converged == 1 and K == 21 and np.sqrt(so.rr) / EPS <= 1 / 3 and before >= 3, (K, before)
    csr = cm.poisson(m)
    with blocks(csr, b, P) as s:
        assert np.array_equal(s.csr_halo(), cm.expected_counts(csr[0], csr[1], P))
        x, st = s.solve(eps=EPS)
        meets_bar(x, st, oracle.poisson_dense(m), b, xo, K)
    no_hip_error()


# ---- 4. every form, the same bits -------------------------------------------------------------------------------
FORMS = [(xchg, fuse, threads) for xchg in ("index", "full", "copy") for fuse in ("1", "0") for threads in ("0", "1")]


def run_forms(s, n, b, monkeypatch):
    """(x, its stats) of the converged solve, checked to be the same bits gated, host-checked, in pieces and a second
    time; and x after a fixed count of 12 from x0 = 0.125."""
    def key(st):
        return (st.iterations, st.converged, np.float64(st.rr).view(np.uint64))
    zero = np.zeros(n)
    x, st = s.solve(x0=zero, eps=EPS)
    assert st.converged == 1
    x2, st2 = s.solve(x0=zero, eps=EPS)  # a second solve on the same context
    assert same_bits(x2, x) and key(st2) == key(st)
    monkeypatch.setenv("CGX_GATED", "0")
    x3, st3 = s.solve(x0=zero, eps=EPS)
    monkeypatch.delenv("CGX_GATED")
    assert same_bits(x3, x) and key(st3) == key(st)
    s.set_x(zero)
    s.begin()
    assert s.iterate(3) == (3, False)
    done, conv = s.iterate(10 * n, eps=EPS)
    assert (3 + done, conv) == (st.iterations, True) and same_bits(s.get_x(), x)
    st4 = s.stats()
    assert key(st4) == key(st)
    xf, stf = s.solve(x0=np.full(n, 0.125), eps=-1.0, max_iter=12)
    assert stf.iterations == 12
    return x, key(st), xf, np.float64(stf.rr).view(np.uint64)


@pytest.mark.parametrize("which", ["masked 1000 over 4", "banded 514 over 2"])
def test_every_form_the_same_bits(which, monkeypatch):
    if which.startswith("masked"):
        n, P, csr, b = 1000, 4, masked(1000, 2)[1], column(1000, 2, 0, 1.0)[0]
    else:
        n, P = 514, 2
        csr, _, b, _ = banded(n)
    seen = {}
    for xchg, fuse, threads in FORMS:
        if xchg == "copy":
            monkeypatch.setenv("CGX_LOCAL_XCHG", "copy")
        else:
            monkeypatch.delenv("CGX_LOCAL_XCHG", raising=False)
            monkeypatch.setenv("CGX_CSR_XCHG", xchg)
        monkeypatch.setenv("CGX_LOCAL_FUSE", fuse)
        monkeypatch.setenv("CGX_LOCAL_THREADS", threads)
        with blocks(csr, b, P) as s:
            flags = s.info.flags
            kernels = xchg != "copy"
            assert bool(flags & HALO_ACTIVE) == (xchg == "index"), (xchg, hex(flags))
            assert bool(flags & cg.CGX_PULL_ACTIVE) == kernels
            assert bool(flags & cg.CGX_FOLDED_ACTIVE) == (kernels and fuse == "1")
            assert bool(flags & cg.CGX_THREADS_ACTIVE) == (kernels and fuse == "1" and threads == "1")
            assert np.array_equal(s.csr_halo(), halo_counts(csr[0], csr[1], P))  # the plan, whatever form runs
            seen[xchg, fuse, threads] = run_forms(s, n, b, monkeypatch)
    first = seen[FORMS[0]]
    for form, got in seen.items():
        assert same_bits(got[0], first[0]) and got[1] == first[1], form
        assert same_bits(got[2], first[2]) and got[3] == first[3], form
    no_hip_error()


# ---- 5. the element-wise probe from a rough x0 ----------------------------------------------------------------------
def snapshots(s):
    """(x after each of the loops 1, 2, 3; the recurrence's r.r after each: rrs[k - 1] belongs to loop k)."""
    s.begin()
    xs, rrs = [], []
    for _ in nq.KS:
        assert s.iterate(1, eps=-1.0) == (1, False)
        xs.append(s.get_x())
        rrs.append(s.stats().rr)
    return xs, rrs


def held_to_reference(col, xs, rrs, what):
    """The worst ratios to the bars of x and of r.r; raises on any element beyond its bar."""
    ref = nq.column(col)
    worst_x, worst_rr, bad = 0.0, 0.0, []
    for k, x in zip(nq.KS, xs):
        q = nq.ratios(x, ref.X[k], ref.S[k]) / nq.bar(col, k)
        worst_x = max(worst_x, float(np.max(q)))
        if not np.all(q <= 1.0):  # NaN included
            rows = np.flatnonzero(~(q <= 1.0))
            bad.append(("x", k, rows.size, [(int(i), float(q[i])) for i in rows[:8]]))
    for k in (k for k in nq.KS if k < col.n):  # past exact convergence r.r is rounding noise
        q = float(abs(nq.LD(rrs[k - 1]) - ref.RR[k]) / ref.T[k]) / nq.rr_bar(col, k)
        worst_rr = max(worst_rr, q)
        if not q <= 1.0:
            bad.append(("rr", k, q))
    assert not bad, (what, "x: loop, elements beyond the bar, the first (row, ratio); rr: loop, ratio", bad)
    return worst_x, worst_rr


PROBES = [(2, 2), (3, 3), (255, 5), (256, 8), (514, 2), (2049, 3), (4097, 17)]


@pytest.mark.parametrize("n,P", PROBES)
def test_probe_from_a_rough_x0(n, P, monkeypatch):
    col = nq.Col("csr", n, 0, False)
    csr = nq.operator("csr", n).csr()
    b, x0 = nq.start(col)
    runs = {}
    for xchg in ("index", "full"):
        monkeypatch.setenv("CGX_CSR_XCHG", xchg)
        with blocks(csr, b, P, x0=x0) as s:
            assert bool(s.info.flags & HALO_ACTIVE) == (xchg == "index")
            xs, rrs = snapshots(s)
            worst = held_to_reference(col, xs, rrs, (n, P, xchg))
            s.set_x(x0)
            again, rrs_again = snapshots(s)  # a second run: the same bits after every loop
            assert all(same_bits(a, x) for a, x in zip(again, xs)) and same_bits(rrs_again, rrs)
            runs[xchg] = (xs, rrs)
            print(f"\n[csr multi probe] n={n} over {P}, {xchg}: x {worst[0]:.3g} of its bar, r.r {worst[1]:.3g}")
    assert all(same_bits(a, x) for a, x in zip(runs["index"][0], runs["full"][0]))
    assert same_bits(runs["index"][1], runs["full"][1])
    no_hip_error()


class Widened:
    """The banded operator of n rows with every entry rounded to float and widened again -- what a float-stored
    context computes with -- as tests/_nrhs_probe.py's operators are: apply in the vector's type, apply_abs."""

    def __init__(self, n):
        base = nq.operator("csr", n).sys

        def wide(a):
            return a.astype(np.float32).astype(np.float64)

        def system(diag, off):
            s = object.__new__(nq.pp.System)
            s.n, s._typed, s.diag, s.off = n, {}, diag, off
            return s
        self.n = n
        self.sys = system(wide(base.diag), {d: wide(c) for d, c in base.off.items()})
        self._abs = system(np.abs(self.sys.diag), {d: np.abs(c) for d, c in self.sys.off.items()})

    def apply(self, p):
        return self.sys.apply(p)

    def apply_abs(self, p):
        return self._abs.apply(p)


def test_probe_float_stored_values():
    """Float-stored values at (514, 2), element-wise: the reference is the same recurrence in long double on the
    widened matrix (the float-rounded entries, exactly what the kernels multiply with), the bars are
    tests/_nrhs_probe.py's rule measured on that matrix: 100 x the spread between its three fp64 summation orders,
    floored at 4 ulp.  Beside them, the contract's bits: a double-valued context over the same blocks on the
    widened values gives the same x and r.r after every loop."""
    n, P = 514, 2
    indptr, indices, data = nq.operator("csr", n).csr()
    b, x0 = nq.start(nq.Col("csr", n, 0, False))
    op = Widened(n)
    wide = op.sys.csr()[2]
    assert np.array_equal(wide, data.astype(np.float32).astype(np.float64)) and not np.array_equal(wide, data)
    X, RR, S, T = nq.cg(op, b, x0, nq.LD, np.dot, True)
    spread, rr_spread = {k: nq.FLOOR for k in nq.KS}, {k: nq.FLOOR for k in nq.KS}
    for dot in nq.DOTS.values():
        Xf, RRf = nq.cg(op, b, x0, np.float64, dot)
        for k in nq.KS:
            spread[k] = max(spread[k], float(np.max(nq.ratios(Xf[k - 1], X[k - 1], S[k - 1]))))
            rr_spread[k] = max(rr_spread[k], float(abs(nq.LD(RRf[k]) - RR[k]) / T[k]))
    assert all(100.0 * v <= nq.CAP for v in list(spread.values()) + list(rr_spread.values()))
    stored, widened = (indptr, indices, data), (indptr, indices, wide)
    with blocks(stored, b, P, x0=x0, a_f32=True) as f, blocks(widened, b, P, x0=x0) as d:
        assert f.info.flags & cg.CGX_A_F32 and not d.info.flags & cg.CGX_A_F32
        assert f.matvec_plan() == d.matvec_plan()
        (xf, rf), (xd, rd) = snapshots(f), snapshots(d)
        worst = 0.0
        for k in nq.KS:
            q = nq.ratios(xf[k - 1], X[k - 1], S[k - 1]) / (100.0 * spread[k])
            qr = float(abs(nq.LD(rf[k - 1]) - RR[k]) / T[k]) / (100.0 * rr_spread[k])
            worst = max(worst, float(np.max(q)), qr)
            assert np.all(q <= 1.0) and qr <= 1.0, (k, float(np.max(q)), qr)
        print(f"\n[csr multi probe] n={n} over {P}, float-stored: worst {worst:.3g} of its bar")
        assert all(same_bits(a, x) for a, x in zip(xf, xd)) and same_bits(rf, rd)
    no_hip_error()


# ---- 6. replacing the matrix ----------------------------------------------------------------------------------------
def test_replacing_the_matrix():
    n, P = 514, 2
    csr, _, b, _ = banded(n)
    indptr, indices, data = csr
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = np.abs(indices - rows) != 37  # the band at 37 removed: shorter lists, still diagonally dominant
    thin = (np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64),
            indices[keep], data[keep])
    assert halo_counts(*csr[:2], P).tolist() == [[0, 37], [37, 0]]
    assert halo_counts(*thin[:2], P).tolist() == [[0, 2], [2, 0]]
    with blocks(thin, b, P) as fresh:
        x_thin, st_thin = fresh.solve(eps=EPS)
        assert st_thin.converged == 1
    with blocks(csr, b, P) as s:
        x_full, st_full = s.solve(eps=EPS)
        assert st_full.converged == 1 and np.array_equal(s.csr_halo(), halo_counts(*csr[:2], P))
        s.set_csr(*thin)
        with pytest.raises(cg.CgxError) as e:  # the call ended the solve in progress
            s.iterate(1)
        assert e.value.code == -6
        assert np.array_equal(s.csr_halo(), halo_counts(*thin[:2], P))
        x, st = s.solve(x0=np.zeros(n), eps=EPS)
        assert same_bits(x, x_thin) and (st.iterations, st.converged) == (st_thin.iterations, 1)
        assert same_bits(st.rr, st_thin.rr) and not same_bits(x, x_full)
        # a column out of range: refused by the structure check, naming the entry
        for bad in (n, -1):
            idx = thin[1].copy()
            idx[idx.size // 2] = bad
            with pytest.raises(cg.CgxError) as e:
                s.set_csr(thin[0], idx, thin[2])
            assert e.value.code == -4 and f"col_idx[{idx.size // 2}] = {bad}" in str(e.value)
        # block 1 above the room every block has (the banded matrix's largest block): explicit zeros at distance 5
        room = int(max(indptr[n // P], indptr[n] - indptr[n // P]))
        extra = np.arange(n // P, n)
        r2 = np.concatenate([rows, extra])
        c2 = np.concatenate([indices, extra - 5]).astype(np.int32)
        v2 = np.concatenate([data, np.zeros(extra.size)])
        order = np.lexsort((c2, r2))
        fat = (np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.int64), c2[order], v2[order])
        count1 = int(fat[0][n] - fat[0][n // P])
        assert count1 > room >= int(fat[0][n // P])
        with pytest.raises(cg.CgxError) as e:
            s.set_csr(*fat)
        assert e.value.code == -4 and "row block 1" in str(e.value) and f"{count1} entries" in str(e.value)
        assert f"room for {room}" in str(e.value)
        # the earlier matrix, its lists and its bits stay
        assert np.array_equal(s.csr_halo(), halo_counts(*thin[:2], P))
        x2, st2 = s.solve(x0=np.zeros(n), eps=EPS)
        assert same_bits(x2, x_thin) and st2.iterations == st_thin.iterations
        # float-stored values replace double ones and back, the lists unchanged
        s.set_csr(*thin, a_f32=True)
        assert s.info.flags & cg.CGX_A_F32 and np.array_equal(s.csr_halo(), halo_counts(*thin[:2], P))
        s.set_csr(*thin)
        x3, _ = s.solve(x0=np.zeros(n), eps=EPS)
        assert not s.info.flags & cg.CGX_A_F32 and same_bits(x3, x_thin)
    no_hip_error()


# ---- 7. lifecycle and refusals on a live context ----------------------------------------------------------------
def test_lifecycle_and_refusals():
    n, P = 1000, 4
    A, csr = masked(n, 2)
    b, xo, K = column(n, 2, 0, 1.0)
    with cg.Solver.csr(n, int(csr[0][-1]), devices=[0] * P, flags=cg.CGX_TIMING) as s:
        info = s.info
        assert (info.nshards, info.nrows, info.n, info.elem_bytes) == (P, n, n, 8)
        assert info.flags & cg.CGX_CSR_ACTIVE and info.flags & HALO_ACTIVE and info.flags & cg.CGX_TIMING
        assert not info.flags & (cg.CGX_FUSED_ACTIVE | cg.CGX_FOLD_ACTIVE | cg.CGX_OVERLAP_ACTIVE | cg.CGX_PEER_ACTIVE)
        assert s.overlap_info()["decided_by"] == "n/a"
        for call in (s.begin, lambda: s.solve(eps=EPS), s.residual_norm, s.csr_halo):
            with pytest.raises(cg.CgxError) as e:  # no matrix yet
                call()
            assert e.value.code == -6

        def refused_everywhere():
            W = np.tile(np.eye(2), (n // 2, 1, 1))
            for call in (lambda: s.set_precond("jacobi"), lambda: s.set_precond(None),
                         lambda: s.set_precond(np.ones(n)), lambda: s.set_precond_block(2),
                         lambda: s.set_precond(("block", 4)), lambda: s.set_precond_block(2, W),
                         s.generate_spd, lambda: s.set_system(A, b), lambda: s.set_rows(0, A_rows=A)):
                with pytest.raises(cg.CgxError) as e:
                    call()
                assert e.value.code == -1, str(e.value)
                assert s.precond == "none"

        refused_everywhere()  # the kind of context decides, before the missing matrix does
        s.set_csr(*csr)
        s.set_rows(0, b_rows=b, x_rows=np.zeros(n))
        refused_everywhere()
        assert not s.info.flags & cg.CGX_PRECOND_ACTIVE
        before = s.matvec_plan()
        for R, U, nt in ((8, 2, 8), (3, 1, 8), (64, 1, 8), (8, 1, 0), (0, 1, 8)):
            with pytest.raises(cg.CgxError) as e:
                s.set_matvec_plan(R, U, nt)
            assert e.value.code == -1 and s.matvec_plan() == before
        x, st = s.solve(eps=EPS)
        meets_bar(x, st, A, b, xo, K)
        rn, bn = s.residual_norm()
        assert abs(rn - np.linalg.norm(b - A @ x)) <= 1e-12 * np.linalg.norm(b)
        assert abs(bn - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
        with pytest.raises(cg.CgxError) as e:  # residual_norm ended the solve
            s.iterate(1)
        assert e.value.code == -6
        s.reset_timing()
        x12, st12 = s.solve(x0=np.zeros(n), eps=-1.0, max_iter=12)  # x0 = 0: no product at the start
        assert st12.iterations == 12 and st12.matvec_count == 12 and st12.matvec_ms > 0.0  # block 0's SpMV, once each
        s.set_matvec_plan(8, 1, 8)  # a chosen plan holds for every block: the solve still meets the bar
        assert (s.matvec_plan()["R"], s.matvec_plan()["nt"]) == (8, 8)
        x8, st8 = s.solve(x0=np.zeros(n), eps=EPS)
        meets_bar(x8, st8, A, b, xo, K)
    with pytest.raises(cg.CgxError) as e:  # any other kind of context has no exchange plan
        with cg.Solver.from_csr(*csr) as one:
            one.csr_halo()
    assert e.value.code == -1
    no_hip_error()


# ---- 8. distinct devices --------------------------------------------------------------------------------------------
def test_distinct_devices():
    visible = cg.device_count()
    if visible < 2:
        pytest.skip(f"{visible} GPU visible: row blocks on distinct devices need at least two")
    G = max(g for g in range(2, min(8, visible) + 1) if 1000 % g == 0)
    csr = masked(1000, 2)[1]
    b = column(1000, 2, 0, 1.0)[0]
    with blocks(csr, b, G) as same:
        x0, st0 = same.solve(eps=EPS)
        assert not same.info.flags & cg.CGX_PEER_ACTIVE
    with blocks(csr, b, G, devices=list(range(G))) as s:
        assert s.info.flags & cg.CGX_PEER_ACTIVE and s.info.flags & HALO_ACTIVE
        x, st = s.solve(eps=EPS)
        assert same_bits(x, x0) and (st.iterations, st.converged) == (st0.iterations, 1) and same_bits(st.rr, st0.rr)
        xf, _ = s.solve(x0=np.full(1000, 0.125), eps=-1.0, max_iter=12)
    with blocks(csr, b, G) as same:
        xf0, _ = same.solve(x0=np.full(1000, 0.125), eps=-1.0, max_iter=12)
    assert same_bits(xf, xf0)
    no_hip_error()
