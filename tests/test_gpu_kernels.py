"""Kernel-level parity (device pointers through the C ABI) on the GPU.

fp32-ref kernels must equal the oracle / numpy float32 bit for bit (the
reference's operation order).  fp64 kernels are checked against the oracle's
sequential fp64 loops with a stated tolerance: a reordered fp64 sum of n
terms differs by at most ~n * 2^-53 * sum|a_i b_i|; we use 1e-13 relative to
sum|a_i b_i| for n <= 8192 (bound 9e-13 worst case, ~1e-15 typical)."""
import functools

import numpy as np
import pytest

import conjugate_gradient_amd as cg
import oracle
import _matvec_order as mo

pytestmark = pytest.mark.gpu

F64_TOL = 1e-13


def dev(a, dtype=None):
    return cg.DeviceArray.from_host(np.ascontiguousarray(a, dtype=dtype))


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


@pytest.mark.parametrize("rows,cols", [(64, 1024), (40, 1000)])
def test_matvec_ref_f32_nonfinite_bitwise(rows, cols):
    """Inf, -Inf and NaN entries flow through the chains as in the reference
    (the zero products the default kernel gives padded columns stay exact)."""
    rng = np.random.default_rng(11)
    A = rng.random((rows, cols), dtype=np.float32) - 0.5
    A[3, 7], A[5, cols - 1], A[rows - 1, 0], A[9, 100] = np.inf, -np.inf, np.nan, 3e38
    v = rng.random(cols, dtype=np.float32) * 4
    out = cg.DeviceArray(rows, np.float32)
    cg.matVec(dev(A), dev(v), out, rows, cols)
    ref = oracle.matvec_f32ref(A, v)
    assert np.array_equal(out.to_host().view(np.uint32), ref.view(np.uint32))


# The 32-row blocks with two 512-column tiles in flight and a dedicated adding wave: their FULL form when
# rows % 32 == 0 and cols % 512 == 0, a bounds-checked form for other multiples of 4; the 16-row kernel
# when cols % 4 != 0 (rows not 16-B aligned).
@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 2), (5, 3), (64, 64), (300, 257), (1000, 1000), (8192, 96),
                                       (16, 512), (17, 513), (33, 1536), (48, 1025), (100, 4100), (32, 512),
                                       (64, 1024), (96, 2560), (31, 4), (33, 516), (1024, 8192), (8192, 8192)])
def test_matvec_ref_f32_bitwise(rows, cols):
    rng = np.random.default_rng(rows * 7 + cols)
    A = rng.random((rows, cols), dtype=np.float32) - 0.5
    v = rng.random(cols, dtype=np.float32)
    out = cg.DeviceArray(rows, np.float32)
    cg.matVec(dev(A), dev(v), out, rows, cols)
    ref = oracle.matvec_f32ref(A, v)
    assert np.array_equal(out.to_host().view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4096, 4097, 8192, 8193, 20000])
def test_dot_ref_f32_bitwise(n):
    rng = np.random.default_rng(n)
    a = rng.random(n, dtype=np.float32) - 0.5
    b = rng.random(n, dtype=np.float32)
    out = cg.DeviceArray(1, np.float32)
    cg.vecVec(dev(a), dev(b), out)
    assert out.to_host()[0].view(np.uint32) == oracle.dot_f32ref(a, b).view(np.uint32)


def test_vector_updates_ref_f32_bitwise():
    rng = np.random.default_rng(3)
    n = 5000
    f = np.float32
    b, Ax, x, p, Ap = (rng.random(n, dtype=f) for _ in range(5))
    r_d, p_d, rr_d = cg.DeviceArray(n, f), cg.DeviceArray(n, f), cg.DeviceArray(1, f)
    cg.residual(dev(b), dev(Ax), r_d, p_d, rr_d)
    r = b - Ax  # numpy float32: one rounding per op, like serialConjugate.c:129
    assert np.array_equal(r_d.to_host(), r) and np.array_equal(p_d.to_host(), r)
    assert rr_d.to_host()[0] == oracle.dot_f32ref(r, r)

    rsold, pAp = np.array([f(2.5)]), np.array([f(7.25)])
    x_d, r2_d, rr2_d = dev(x), dev(r), cg.DeviceArray(1, f)
    cg.update_xr(x_d, r2_d, dev(p), dev(Ap), dev(rsold), dev(pAp), rr2_d)
    alpha = f(rsold[0] / pAp[0])
    x_ref = x + p * alpha
    r_ref = r - Ap * alpha
    assert np.array_equal(x_d.to_host(), x_ref) and np.array_equal(r2_d.to_host(), r_ref)
    assert rr2_d.to_host()[0] == oracle.dot_f32ref(r_ref, r_ref)

    p_d2 = dev(p)
    cg.update_p(p_d2, dev(r_ref), dev(np.array([f(1.5)])), dev(rsold))
    ratio = f(f(1.5) / rsold[0])
    assert np.array_equal(p_d2.to_host(), r_ref + p * ratio)


@pytest.mark.parametrize("rows,cols,lda", [(1, 1, 1), (3, 5, 5), (7, 129, 131), (128, 128, 128),
                                           (1000, 1000, 1000), (4096, 4096, 4096), (33, 8192, 8200),
                                           (20000, 256, 256)])
def test_matvec_f64(rows, cols, lda):
    rng = np.random.default_rng(rows + cols)
    A = rng.random((rows, lda)) - 0.5
    v = rng.random(cols)
    out = cg.DeviceArray(rows, np.float64)
    cg.matVec(dev(A), dev(v), out, rows, cols, lda)
    ref = oracle.matvec_f64(np.ascontiguousarray(A[:, :cols]), v)
    scale = np.abs(A[:, :cols]) @ np.abs(v)
    assert np.all(np.abs(out.to_host() - ref) <= F64_TOL * scale + 1e-300)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100000, 1 << 20])
def test_dot_and_updates_f64(n):
    rng = np.random.default_rng(n)
    a, b = rng.random(n) - 0.5, rng.random(n)
    out = cg.DeviceArray(1, np.float64)
    cg.vecVec(dev(a), dev(b), out)
    assert abs(out.to_host()[0] - a @ b) <= F64_TOL * (np.abs(a) @ np.abs(b))
    # deterministic: the same launch twice gives the same bits
    cg.vecVec(dev(a), dev(b), out)
    first = out.to_host()[0]
    cg.vecVec(dev(a), dev(b), out)
    assert out.to_host()[0] == first

    x, r, p, Ap = (rng.random(n) for _ in range(4))
    x_d, r_d, rr_d = dev(x), dev(r), cg.DeviceArray(1, np.float64)
    cg.update_xr(x_d, r_d, dev(p), dev(Ap), dev(np.array([3.0])), dev(np.array([4.0])), rr_d)
    alpha = 0.75
    np.testing.assert_allclose(x_d.to_host(), x + alpha * p, rtol=1e-15, atol=0)
    r_ref = r - alpha * Ap
    np.testing.assert_allclose(r_d.to_host(), r_ref, rtol=1e-13, atol=1e-15)
    assert abs(rr_d.to_host()[0] - r_ref @ r_ref) <= F64_TOL * (r_ref @ r_ref)


# every plan libcgx ships: R rows per wave x U chunks in flight x load policy
# (0 plain, 1 non-temporal, 2 / 8 pipelined plain / non-temporal = default); R=8 U=8
# pipelined spills and is never planned
MV_PLANS = [(R, U, nt) for R in (1, 2, 4, 8) for U in (2, 4, 8) for nt in (0, 1, 2, 8)
            if not (R == 8 and U == 8 and nt in (2, 8))]


@pytest.mark.parametrize("rows,cols", [(300, 2048), (2048, 4096), (5000, 5120), (8192, 8192), (77, 2560)])
def test_matvec_small_lds_bitwise_equals_l2_kernel(monkeypatch, rows, cols):
    """k_matvec_small_f64 (the vector staged in LDS, one block per CU; the
    solver's matVec on one GPU at 2048 <= lda <= 8192) sums every row as
    k_matvec_f64 does -- per lane, chunks in ascending order, then the wave
    sum -- so Ap is bit for bit the L2 kernel's: rows fewer than the grid's
    waves (77, 300), several rows per wave (5000, 8192), 4 chunks per step
    (2560 = 20 chunks).  CGX_MV_SMALL=2 routes the kernel-level cgx_matvec
    through it."""
    rng = np.random.default_rng(rows * 7 + cols)
    A = rng.random((rows, cols)) - 0.5
    v = rng.random(cols)
    A_d, v_d = dev(A), dev(v)
    out = cg.DeviceArray(rows)
    cg.matVec(A_d, v_d, out, rows, cols)
    base = out.to_host()
    assert np.all(np.abs(base - oracle.matvec_f64(A, v)) <= F64_TOL * (np.abs(A) @ np.abs(v)))
    monkeypatch.setenv("CGX_MV_SMALL", "2")
    for nt, u in (("512", "8"), ("512", "4"), ("1024", "4"), ("1024", "8")):
        monkeypatch.setenv("CGX_SMALL_PLAN", f"threads={nt},U={u}")
        out = cg.DeviceArray(rows)
        cg.matVec(A_d, v_d, out, rows, cols)
        assert np.array_equal(out.to_host(), base), (nt, u)


@pytest.mark.parametrize("rows,cols", [(300, 1000), (1000, 1024), (517, 2176), (2048, 4096), (8192, 3200)])
def test_matvec_f64_every_plan_bitwise_equal(monkeypatch, rows, cols):
    """Every (rows per wave, chunks in flight, load policy) plan, including the
    software-pipelined kernel (8) with chunk counts that are not a multiple of
    U, gives the same row sums bit for bit: each lane accumulates its columns
    in ascending order whatever the plan.  The default plan is checked against
    the fp64 oracle.  (The rejected variants are checked the same way by
    tools/microbench/matvec_variants.hip.)"""
    rng = np.random.default_rng(rows + cols)
    A = rng.random((rows, cols)) - 0.5
    v = rng.random(cols)
    A_d, v_d = dev(A), dev(v)
    ref = oracle.matvec_f64(A, v)
    out = cg.DeviceArray(rows)
    cg.matVec(A_d, v_d, out, rows, cols)
    base = out.to_host()
    bound = F64_TOL * (np.abs(A) @ np.abs(v))
    assert np.all(np.abs(base - ref) <= bound)
    for R, U, nt in MV_PLANS:
        monkeypatch.setenv("CGX_MV_PLAN", f"R={R},U={U},nt={nt}")
        out = cg.DeviceArray(rows)
        cg.matVec(A_d, v_d, out, rows, cols)
        assert np.array_equal(out.to_host(), base), (R, U, nt)


# The summation order itself, stated on the CPU (_matvec_order.py): the tests above compare plan with plan
# and kernel with kernel, so a change of order in code they all share would pass them.  (cols, lda, v's
# offset in doubles from the 16-byte grid); shapes: _matvec_order.py.  A v 8 bytes off the grid or an odd
# pitch sends every column through the scalar tail -- so does lda = cols for an odd cols, and those sizes
# run with the pitch rounded up to even as well: that is where their chunks, remainders and tails meet.
ORDER_F64 = ([(c, c, 0) for c in mo.F64_COLS] + [(c, c + 1, 0) for c in mo.F64_COLS if c % 2] +
             [(389, 389, 1), (389, 390, 1), (389, 391, 0)])


@functools.lru_cache(maxsize=None)
def order_f64(cols, lda, vector_path):
    A, v = mo.f64_case(cols, lda)
    return A, v, np.array(mo.matvec_f64(A, v, cols, cols & ~127 if vector_path else 0))


def matvec_at(dtype, A, v, voff, cols, lda):
    """Kernel-level cgx_matvec on A and on v placed voff doubles into a device array; (out, A's and v's address)."""
    dA, dv, out = dev(A), dev(np.concatenate([np.zeros(voff), v])), cg.DeviceArray(mo.ROWS)
    L = cg.lib()
    assert L.cgx_matvec(dtype, dA.ptr, lda, mo.ROWS, cols, dv.ptr + 8 * voff, out.ptr, None) == 0, L.cgx_last_error()
    assert L.cgx_dev_synchronize() == 0, L.cgx_last_error()
    return out.to_host(), dA.ptr, dv.ptr + 8 * voff


@pytest.mark.parametrize("plan", [None, "R=4,U=4,nt=8", "R=1,U=2,nt=0"])
@pytest.mark.parametrize("cols,lda,voff", ORDER_F64)
def test_matvec_f64_is_the_documented_order(monkeypatch, cols, lda, voff, plan):
    """k_matvec_f64's row sums are the CPU emulation of the documented order bit for bit, under the default
    plan, a four-rows-per-wave pipelined plan and an unpipelined one (the other plans: the every-plan test)."""
    monkeypatch.delenv("CGX_MV_SMALL", raising=False)
    if plan:
        monkeypatch.setenv("CGX_MV_PLAN", plan)
    else:
        monkeypatch.delenv("CGX_MV_PLAN", raising=False)
    A, v, want = order_f64(cols, lda, voff == 0 and lda % 2 == 0)
    got, pa, pv = matvec_at(cg.CGX_F64, A, v, voff, cols, lda)
    assert mo.vec_cols_f64(cols, pa, pv, lda) == (cols & ~127 if voff == 0 and lda % 2 == 0 else 0)
    assert np.array_equal(got, want), np.flatnonzero(got != want)


@pytest.mark.parametrize("cols", [2048, 2560])
def test_matvec_small_lds_is_the_documented_order(monkeypatch, cols):
    """k_matvec_small_f64 (CGX_MV_SMALL=2 routes cgx_matvec through it) likewise: 16 chunks per row run with
    U = 8, 20 with U = 4."""
    monkeypatch.setenv("CGX_MV_SMALL", "2")
    monkeypatch.delenv("CGX_SMALL_PLAN", raising=False)
    monkeypatch.delenv("CGX_MV_PLAN", raising=False)
    A, v, want = order_f64(cols, cols, True)
    got, _, _ = matvec_at(cg.CGX_F64, A, v, 0, cols, cols)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    # that the call above took the LDS-staged kernel: it refuses a v off the 16-byte grid on the host side,
    # where k_matvec_f64 would send every column through its scalar tail and succeed
    dA, dv, out = dev(A), dev(np.concatenate([np.zeros(1), v])), cg.DeviceArray(mo.ROWS)
    assert cg.lib().cgx_matvec(cg.CGX_F64, dA.ptr, cols, mo.ROWS, cols, dv.ptr + 8, out.ptr, None) != 0


# ---- the fp64 BLAS-1 kernels at their edges ------------------------------------------------------
# Reference: the same operation in np.longdouble.  a + s*b elementwise: |got - ref| <= 2^-52 (|a_i| + |s b_i|),
# which covers the fused and the two-rounding evaluation; the scalar pairs (3/4, 5/8) have exact quotients.
# Reductions: F64_TOL relative to sum|a_i b_i| (no term passes through more than ~64 additions here: a per-thread
# chain, 6 wave steps, 4 waves, a partial chain of at most 8, the same again -- 7e-15).
# Sizes: 2048 = one block's VEC span; 4196355 = 2048 * 2048 + 2051 takes the VEC grid-stride loop into a partial
# second trip with an odd tail; 100001 wraps the scalar form's loop eight times.
# Placement: every kernel has a VEC form (every pointer 16-byte aligned) and a scalar form; one operand 8 bytes
# off the grid must select the scalar form for all of them.
EDGE_N = [1, 2, 3, 255, 2047, 2048, 2049, 4097, 100001, 4196355]
GUARD = 2  # sentinel elements on each side of a placed vector (16 bytes: the placement's phase is kept)
SENTINEL = np.float64(-1.2345e300)
EPS52 = 2.0 ** -52


def ld(a):
    return np.asarray(a, np.longdouble)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Placed:
    """A device vector `off` elements (0 or 1) past a 16-byte boundary, inside an array one element longer,
    with sentinels before and after it; get() returns it after checking that every sentinel is untouched."""

    def __init__(self, host, off):
        host = np.atleast_1d(np.asarray(host, np.float64))
        self.lo, self.hi = GUARD + off, GUARD + off + host.size
        buf = np.full(GUARD + 1 + host.size + GUARD, SENTINEL)
        buf[self.lo:self.hi] = host
        self.d = dev(buf)
        self.ptr = self.d.ptr + 8 * self.lo
        assert (self.ptr % 16 == 0) == (off == 0)

    def get(self):
        buf = self.d.to_host()
        out = np.concatenate([buf[:self.lo], buf[self.hi:]])
        assert same_bits(out, np.full(out.size, SENTINEL)), "a guard element was written"
        return buf[self.lo:self.hi]


def placements(nops, n):
    """(name, offsets): all aligned (VEC), all +8 (scalar), exactly one operand +8 (scalar for all) -- each
    operand in turn at the small sizes, one of them at the large ones."""
    yield "aligned", (0,) * nops
    yield "all+8", (1,) * nops
    for i in (range(nops) if n <= 5000 else [n % nops]):
        yield f"only operand {i} +8", tuple(int(j == i) for j in range(nops))


def call(name, *args):
    """A CGX_F64 entry point on Placed vectors (kept alive here until the launch has finished), None or ints."""
    L = cg.lib()
    rc = getattr(L, name)(cg.CGX_F64, *(a.ptr if isinstance(a, Placed) else a for a in args), None)
    assert rc == 0, (name, L.cgx_last_error())
    assert L.cgx_dev_synchronize() == 0, (name, L.cgx_last_error())


def sum_close(got, terms):
    """got == sum(terms) to F64_TOL * sum|terms|, the sum taken in long double."""
    t = ld(terms)
    return abs(np.longdouble(got) - t.sum()) <= F64_TOL * np.abs(t).sum()


@pytest.mark.parametrize("n", EDGE_N)
def test_residual_f64_edges(n):
    """cgx_residual(CGX_F64): r and p both written and equal, rr = r.r; rr_dev = NULL leaves r and p correct."""
    rng = np.random.default_rng(n)
    b, Ax = rng.random(n) - 0.5, rng.random(n) - 0.5
    ref = ld(b) - ld(Ax)
    bound = EPS52 * (np.abs(b) + np.abs(Ax))
    for name, (ob, oa, orr, op) in placements(4, n):
        runs = []
        for with_rr in (True, True, False):
            b_d, a_d = Placed(b, ob), Placed(Ax, oa)
            r_d, p_d, rr_d = Placed(np.full(n, np.nan), orr), Placed(np.full(n, np.nan), op), Placed(np.nan, 0)
            call("cgx_residual", n, b_d, a_d, r_d, p_d, rr_d if with_rr else None)
            runs.append((r_d.get(), p_d.get(), rr_d.get()[0]))
            assert same_bits(b_d.get(), b) and same_bits(a_d.get(), Ax), name
        r, p, rr = runs[0]
        assert same_bits(r, p) and np.all(np.abs(ld(r) - ref) <= bound), name
        assert sum_close(rr, ld(r) * ld(r)), (name, rr)
        assert same_bits(runs[1][0], r) and same_bits(runs[1][1], r) and runs[1][2] == rr, name  # deterministic
        assert same_bits(runs[2][0], r) and same_bits(runs[2][1], r) and np.isnan(runs[2][2]), name


@pytest.mark.parametrize("n", EDGE_N)
def test_update_p_f64_edges(n):
    """cgx_update_p(CGX_F64): p = r + (5/8) p elementwise; r untouched.  (Never called with CGX_F64 outside a
    solve before; the odd-tail line of the VEC form is reached only here and in 4-iteration solves.)"""
    rng = np.random.default_rng(n + 1)
    p, r = rng.random(n) - 0.5, rng.random(n) - 0.5
    beta = 0.625
    ref = ld(r) + np.longdouble(beta) * ld(p)
    bound = EPS52 * (np.abs(r) + np.abs(beta * p))
    for name, (op, orr) in placements(2, n):
        got = []
        for _ in range(2):
            p_d, r_d = Placed(p, op), Placed(r, orr)
            call("cgx_update_p", n, p_d, r_d, Placed(5.0, 0), Placed(8.0, 0))
            got.append(p_d.get())
            assert same_bits(r_d.get(), r), name
        assert np.all(np.abs(ld(got[0]) - ref) <= bound), (name, np.abs(ld(got[0]) - ref).max())
        assert same_bits(got[0], got[1]), name


@pytest.mark.parametrize("n", EDGE_N)
def test_update_xr_f64_edges(n):
    """cgx_update_xr(CGX_F64): x += (3/4) p, r -= (3/4) Ap, rr = r.r; p and Ap unchanged."""
    rng = np.random.default_rng(n + 2)
    x, r, p, Ap = (rng.random(n) - 0.5 for _ in range(4))
    alpha = 0.75
    x_ref, r_ref = ld(x) + np.longdouble(alpha) * ld(p), ld(r) - np.longdouble(alpha) * ld(Ap)
    xb, rb = EPS52 * (np.abs(x) + np.abs(alpha * p)), EPS52 * (np.abs(r) + np.abs(alpha * Ap))
    for name, (ox, orr, op, oa) in placements(4, n):
        got = []
        for _ in range(2):
            x_d, r_d, p_d, a_d, rr_d = Placed(x, ox), Placed(r, orr), Placed(p, op), Placed(Ap, oa), Placed(np.nan, 0)
            call("cgx_update_xr", n, x_d, r_d, p_d, a_d, Placed(3.0, 0), Placed(4.0, 0),
                 rr_d)
            got.append((x_d.get(), r_d.get(), rr_d.get()[0]))
            assert same_bits(p_d.get(), p) and same_bits(a_d.get(), Ap), name
        xg, rg, rr = got[0]
        assert np.all(np.abs(ld(xg) - x_ref) <= xb) and np.all(np.abs(ld(rg) - r_ref) <= rb), name
        assert sum_close(rr, ld(rg) * ld(rg)), (name, rr)
        assert same_bits(got[1][0], xg) and same_bits(got[1][1], rg) and got[1][2] == rr, name


@pytest.mark.parametrize("n", EDGE_N)
def test_dot_f64_edges(n):
    rng = np.random.default_rng(n + 3)
    a, b = rng.random(n) - 0.5, rng.random(n) - 0.5
    for name, (oa, ob) in placements(2, n):
        got = []
        for _ in range(2):
            a_d, b_d, out = Placed(a, oa), Placed(b, ob), Placed(np.nan, 0)
            call("cgx_dot", n, a_d, b_d, out)
            got.append(out.get()[0])
            assert same_bits(a_d.get(), a) and same_bits(b_d.get(), b), name
        assert sum_close(got[0], ld(a) * ld(b)), (name, got[0])
        assert got[0] == got[1], name


@pytest.mark.parametrize("off", [0, 1])
def test_cg_ratio_cases_f64(off):
    """cg_ratio's three cases at the kernel level (include/cgx.h, "Iterations past exact convergence";
    test_indefinite_breakdown_is_not_hidden sees the last through a whole solve): 0/0 and a subnormal numerator
    over 0 give 0 -- x and r stay bit for bit; a normal numerator over 0 is the plain quotient, Inf."""
    n = 257
    rng = np.random.default_rng(257)
    x, r, p, Ap = (rng.random(n) - 0.5 for _ in range(4))
    p[[0, 100, 256]] = 0.0, -0.0, 0.0  # the odd tail among them
    for rsold in (0.0, 5e-324):
        x_d, r_d, rr_d = Placed(x, off), Placed(r, off), Placed(np.nan, 0)
        call("cgx_update_xr", n, x_d, r_d, Placed(p, off), Placed(Ap, off), Placed(rsold, 0),
             Placed(0.0, 0), rr_d)
        assert same_bits(x_d.get(), x) and same_bits(r_d.get(), r), rsold
        assert sum_close(rr_d.get()[0], ld(r) * ld(r)), rsold
    x_d, r_d, rr_d = Placed(x, off), Placed(r, off), Placed(np.nan, 0)
    call("cgx_update_xr", n, x_d, r_d, Placed(p, off), Placed(Ap, off), Placed(1.0, 0),
         Placed(0.0, 0), rr_d)
    xg = x_d.get()
    assert not np.isfinite(xg).any()
    assert np.array_equal(np.isnan(xg), p == 0.0)
    live = p != 0.0
    assert np.all(np.isinf(xg[live])) and np.array_equal(np.sign(xg[live]), np.sign(p[live]))
    p_d = Placed(p, off)
    call("cgx_update_p", n, p_d, Placed(r, off), Placed(0.0, 0), Placed(0.0, 0))
    assert np.array_equal(p_d.get(), r)  # beta = 0: p == r
