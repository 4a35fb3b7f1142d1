"""Element-wise probes of the preconditioned CG kernels of CSR contexts (csrc/cgx_pcg.hip, csrc/cgx_pcg_block.hip).

Every run is three fixed loops (begin, then iterate(1, eps=-1) three times, x read after each) from a rough x0 and
from x0 = 0 on a rough b, compared element by element with the same loops in long double (tests/_pcg_probe.py, whose
docstring holds the systems, the per-element scale S and the measured bars): |x[i] - x_ld[i]| <= bar S_k[i] for every i,
bar = 100 x the spread between fp64 summation orders.  x_1 shows the start kernel's z row by row, x_2 and x_3 the z the
r update stores and the x/p update's read of it.  The blocks W are not symmetric, and a short last block's unused slots
hold NaN: a transposed layout, a wrong row walk or a read of an unused slot moves some element by at least 1000 bars
(tests/test_pcg_probe_cpu.py runs those mutations on the CPU).

  a. every block size 2..8 with every short last block t = 0..bs-1 at n = 257 bs + t (two thread blocks of W's blocks,
     the short one on a lane of its own), one case also at T = 2; n = bs - 1 (one short block);
  b. the diagonal kinds at the edges of the pair loop (1024 pairs per thread block pass, an odd tail on thread 0);
  c. the grid-stride passes: more than 2048 * 256 blocks of W, more than 2048 * 1024 pairs (x0 rough only: the two
     starts differ in one operand, not in the loop);
  d. blocks with only the diagonal set against CGX_PC_DIAG with the same values: one reference, one bar.

Beside the bar every run asserts: a second run gives the same bits after every loop, and solve(eps=-1, max_iter=3)
the third loop's bits.  Each test prints its worst measured ratio to the bar (pytest -s)."""
import numpy as np
import pytest

import _pcg_probe as pp
import conjugate_gradient_amd as cg

pytestmark = pytest.mark.gpu
BOTH = (False, True)  # x0 rough, x0 = 0


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"
    assert getattr(cg.Solver, "set_precond_block", None) is not None, "the package has no block preconditioner"


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def no_hip_error():
    assert cg.lib().cgx_hip_last_error() == 0


def snapshots(s):
    """x after each of the loops 1, 2, 3 of a fixed-count solve from the context's b and x."""
    s.begin()
    out = []
    for _ in pp.KS:
        assert s.iterate(1) == (1, False)
        out.append(s.get_x())
    return out


def probe(s, sys_, case, what):
    """The probe of `case` on the context s (its matrix and preconditioner set): every element of x after every loop
    to the bar, then the bits of a second run and of the one-call form."""
    pr = pp.probe(case)
    x0 = np.zeros(case.n) if case.zero else sys_.x0
    s.set_rows(0, b_rows=sys_.b, x_rows=x0)
    xs = snapshots(s)
    worst, bad = {}, []
    for k, x in zip(pp.KS, xs):
        q = pp.ratios(x, pr.X[k], pr.S[k]) / pp.bar(case, k)
        worst[k] = float(np.max(q))
        if not np.all(q <= 1.0):  # NaN included
            rows = np.flatnonzero(~(q <= 1.0))
            bad.append((k, rows.size, [(int(i), float(q[i])) for i in rows[:8]]))
    print(f"\n[pcg probe] {what} x0 {'0' if case.zero else 'rough'}: "
          + ", ".join(f"k={k} {v:.3g} of the bar {pp.bar(case, k):.3g}" for k, v in worst.items()))
    assert not bad, (what, case, "loop, rows beyond the bar, the first (row, ratio to the bar)", bad)
    s.set_rows(0, x_rows=x0)
    again = snapshots(s)
    assert all(same_bits(a, x) for a, x in zip(again, xs))
    x3, st = s.solve(x0=x0, eps=-1.0, max_iter=max(pp.KS))
    assert st.iterations == max(pp.KS) and same_bits(x3, xs[-1])


def run_block(n, bs, variants=BOTH, plan=None):
    sys_ = pp.system(n)
    ref, given = pp.blocks(n, bs)
    with cg.Solver.from_csr(*sys_.csr()) as s:
        if plan:
            s.set_matvec_plan(*plan)
        s.set_precond_block(bs, values=given)
        assert s.precond == "block"
        got_bs, got = s.precond_block
        # the used entries bit for bit, +0.0 in the unused slots that were handed in as NaN
        assert got_bs == bs and np.isnan(given).sum() == bs * bs - (n - (len(ref) - 1) * bs) ** 2
        assert same_bits(got, ref)
        for zero in variants:
            probe(s, sys_, pp.Case("block", bs, n, zero), f"bs {bs} n {n}" + (f" plan {plan}" if plan else ""))
    no_hip_error()


# ---- a. every block size, every short block ----------------------------------------------------------------------------
@pytest.mark.parametrize("bs,t", pp.BLOCK_CASES)
def test_block_probe(bs, t):
    n = pp.block_n(bs, t)
    assert pp.nblocks(n, bs) == 257 + (t > 0) and n % bs == t
    run_block(n, bs)
    if (bs, t) == (5, 3):  # once more at T = 2: the bar does not depend on the plan
        run_block(n, bs, plan=(32, 1, 8))


@pytest.mark.parametrize("bs", pp.BLOCK_SIZES)
def test_block_probe_one_short_block(bs):
    run_block(bs - 1, bs)  # n < bs; bs = 2: one row


# ---- c. the grid-stride pass of the block kernels ------------------------------------------------------------------------
def test_block_probe_grid_stride():
    """nblk = 524290 > 2048 * 256: blocks 524288 and 524289 are reached by the stride alone, the second is the short
    one (one row), and n is odd for the x/p kernel's tail."""
    bs, n = pp.BLOCK_STRIDE
    assert pp.nblocks(n, bs) == 2048 * 256 + 2 and n % bs == 1
    run_block(n, bs, variants=(False,))


# ---- b. the diagonal kinds ---------------------------------------------------------------------------------------------
def run_diag(kind, n, variants=BOTH):
    sys_ = pp.system(n)
    case = pp.Case(kind, 0, n, False)
    with cg.Solver.from_csr(*sys_.csr(), precond=pp.library_precond(case)) as s:
        assert s.precond == kind
        want = 1.0 / sys_.diag if kind == "jacobi" else pp.minv(n, "diag")
        assert same_bits(s.precond_diag(), want)
        for zero in variants:
            probe(s, sys_, case._replace(zero=zero), f"{kind} n {n}")
    no_hip_error()


@pytest.mark.parametrize("n", pp.DIAG_SIZES)
@pytest.mark.parametrize("kind", pp.DIAG_KINDS)
def test_diag_probe(kind, n):
    run_diag(kind, n)


def test_diag_probe_grid_stride():
    """n / 2 = 2048 * 1024 + 1 pairs: the last pair is reached by the stride alone, and n is odd."""
    assert pp.DIAG_STRIDE // 2 == 2048 * 1024 + 1 and pp.DIAG_STRIDE % 2 == 1
    run_diag("diag", pp.DIAG_STRIDE, variants=(False,))


# ---- d. diagonal blocks and the diagonal kind, one reference -------------------------------------------------------------
@pytest.mark.parametrize("bs", pp.DIAGONAL_BLOCK_SIZES)
def test_diagonal_blocks_match_the_diagonal_kind_elementwise(bs):
    """The header promises the same z bits, but the dots' orders differ: each is held to the reference, not to the
    other."""
    n = pp.block_n(bs, 1)
    sys_ = pp.system(n)
    W, m = pp.diagonal_blocks(n, bs), pp.minv(n, "diag")
    with cg.Solver.from_csr(*sys_.csr()) as s:
        s.set_precond_block(bs, values=W)
        assert s.precond == "block" and same_bits(s.precond_block[1], np.nan_to_num(W))
        for zero in BOTH:
            probe(s, sys_, pp.Case("diag", 0, n, zero), f"diagonal blocks bs {bs} n {n}")
        s.set_precond(m)
        assert s.precond == "diag" and same_bits(s.precond_diag(), m)
        for zero in BOTH:
            probe(s, sys_, pp.Case("diag", 0, n, zero), f"diag n {n}")
    no_hip_error()
