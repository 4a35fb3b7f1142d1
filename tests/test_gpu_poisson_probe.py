"""Kernel-level probes of the matrix-free Poisson path (csrc/cgx_poisson.hip) on rough data.

Every solve is a fixed count (begin, then iterate(K, eps=-1)) compared element by element with K loops of
sequential CG in long double (tests/_poisson_probe.py), to bar(m, K) = 100 x the measured spread between fp64
summation orders, as a fraction of max|x_ld|.  A neighbour taken from the wrong place moves a point by about
alpha |v| ~ 0.1 max|x|: ten or more orders above the bar.

  a. rough data (standard-normal b and x0: the initial stencil runs, x's halo rows differ between slabs) on
     every shape and form, K = 1, 2, 3 (each residue of the x deferral, the flush with one and two p slabs)
     and 9, with the true residual;
  b. the comb (isolated ones next to every item, wave, strip, slab and grid edge): x == b / 4 bit for bit
     after one loop, exactly zero outside the diamonds after two and three, under every halo exchange form;
  c. every key of CGX_POISSON_PLAN, several items per block included: bit for bit across rb, to the bar for
     the others, every plan twice with equal bits;
  d. the plans stop at the oracle's loop count where the oracle alone keeps a factor of 3 round eps.

Each test prints its worst measured ratio to the bar (pytest -s).

What value tests cannot see: the step parity `par` of the LDS edge buffer guards a write-after-read hazard
between two steps of one block, not a value.  With the toggle taken out of poisson_p_body (a scratch build)
every test here and every Poisson test of test_gpu_solver.py still passed on an MI355X: a wave reaches its
next edge store only after a step's arithmetic and stores, long after the other waves' two LDS reads.
"""
import numpy as np
import pytest

import _poisson_probe as pp
import conjugate_gradient_amd as cg

pytestmark = pytest.mark.gpu
TOL = 1e-10

# (m, devices): one-row slabs (m = 2 / 2, 8 / 8), m = 2 alone, odd m over slabs (k_stencil5_rows_f64 with halos), a
# last strip of one column pair (514, 1026: lane 0 of wave 0 alone, its left point through has_l), three strips
# (1026: the middle one has both outer side points; the split stencil marches two rows per block), full strips
# over two slabs (1024: the pipelined catch-up)
SHAPES = [(2, None), (2, [0, 0]), (8, [0] * 8), (9, [0] * 3), (130, [0, 0]), (514, None), (514, [0, 0]),
          (1024, [0, 0]), (1026, None)]
# form -> (CGX_POISSON_FUSED, CGX_POISSON_XDEFER; None: unset)
FORMS = {"x3": ("1", None), "x2": ("1", "2"), "x1": ("1", "0"), "split": ("0", None)}
# halo exchange form -> (CGX_LOCAL_XCHG, CGX_LOCAL_FUSE, CGX_HALO_OVERLAP)
XCHG = {"pull": (None, None, None), "nofuse": (None, "0", None), "copy-overlap": ("copy", None, "1"),
        "copy": ("copy", None, "0")}


def _id(m, devices):
    return f"m{m}" + (f"x{len(devices)}" if devices else "")


CASES = [pytest.param(m, d, f, id=f"{_id(m, d)}-{f}") for m, d in SHAPES for f in FORMS if m % 2 == 0 or f == "split"]


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


class Worst:
    """The worst measured ratio to each bar within one test, printed at its end; `bad` lists what missed."""

    def __init__(self, what):
        self.what, self.r, self.bad = what, {}, []

    def ratio(self, bar, value, bound, where=""):
        q = float(value) / float(bound)
        self.r[bar] = max(self.r.get(bar, 0.0), q)
        if not q <= 1.0:
            self.bad.append((bar, where, f"{q:.3g} x the bar"))
        return q <= 1.0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        print(f"\n[probe] {self.what}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.r.items()))


def _setenv(monkeypatch, **kv):
    for k, v in kv.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def solver(monkeypatch, m, devices, form, xchg="pull", plan=None):
    """A Poisson context of the given form, after asserting that its flags say what will run."""
    fused, xdefer = FORMS[form]
    lx, lf, ho = XCHG[xchg]
    _setenv(monkeypatch, CGX_POISSON_FUSED=fused, CGX_POISSON_XDEFER=xdefer, CGX_LOCAL_XCHG=lx, CGX_LOCAL_FUSE=lf,
            CGX_HALO_OVERLAP=ho, CGX_POISSON_PLAN=plan, CGX_GATED=None)
    s = cg.Solver(None, poisson_m=m, devices=devices)
    fl = s.info.flags
    try:
        assert bool(fl & cg.CGX_FUSED_ACTIVE) == (form != "split")
        assert bool(fl & cg.CGX_XDEFER_ACTIVE) == (form in ("x3", "x2"))
        assert bool(fl & cg.CGX_XDEFER3_ACTIVE) == (form == "x3")
        if devices and form != "split":
            assert bool(fl & cg.CGX_HALO_PULL_ACTIVE) == (xchg in ("pull", "nofuse"))
            assert bool(fl & cg.CGX_HALO_OVERLAP_ACTIVE) == (xchg == "copy-overlap")
    except AssertionError:
        s.close()
        raise
    return s


def fixed(s, b, x0, K):
    """x, the recurrence's r.r, and (||b - A x||, ||b||) after K fixed loops from (b, x0)."""
    s.set_rows(0, None, b, x0)
    s.begin()
    s.iterate(K, eps=-1.0)
    x = s.get_x()
    rr = s.stats().rr
    return x, rr, s.residual_norm()


def elementwise(w, name, x, x_ld, bar, where=None, note=""):
    """max|x - x_ld| <= bar max|x_ld| over the points `where` (all of them by default)."""
    d = np.abs(x.astype(pp.LD) - x_ld)
    if where is not None:
        d = d[where]
    worst = int(np.argmax(d))
    return w.ratio(name, d[worst], bar * np.max(np.abs(x_ld)), f"{note} worst point {worst}")


@pytest.mark.parametrize("m,devices,form", CASES)
def test_rough_elementwise(monkeypatch, m, devices, form):
    """x after K = 1, 2, 3, 9 fixed loops from rough (b, x0), element by element against long-double CG, and
    the true residual ||b - A x|| and ||b|| against the reference's, to bar(m, K) ||b||."""
    b, x0 = pp.rough(m, m)
    with Worst(f"rough {_id(m, devices)} {form}") as w, solver(monkeypatch, m, devices, form) as s:
        for K in pp.KS:
            x_ld, rn_ld, bn_ld = pp.reference(m, "rough", K)
            x, _, (rn, bn) = fixed(s, b, x0, K)
            bar = pp.bar(m, K)
            assert np.all(np.isfinite(x))
            elementwise(w, "x", x, x_ld, bar, note=f"K={K}")
            w.ratio("residual", abs(pp.LD(rn) - rn_ld), bar * bn_ld, f"K={K}")
            w.ratio("|b|", abs(pp.LD(bn) - bn_ld), bar * bn_ld, f"K={K}")
    assert not w.bad, w.bad


@pytest.mark.parametrize("m,devices,form", [c for c in CASES if c.values[0] >= 8])
def test_comb_exact(monkeypatch, m, devices, form):
    """Isolated ones next to every edge: after one loop x == b / 4 bit for bit; after two and three x is
    exactly 0 outside the radius-(K-1) diamonds (no stray store, no halo or strip-edge read of a point that is
    no neighbour) and agrees with long-double CG inside them.  Several slabs: under every halo exchange."""
    mloc = m // len(devices) if devices else m
    with Worst(f"comb {_id(m, devices)} {form}") as w:
        for xchg in (XCHG if devices else ("pull",)):
            with solver(monkeypatch, m, devices, form, xchg) as s:
                for K in (1, 2, 3):
                    b, x0, mask = pp.comb(m, mloc, K)
                    x, _, _ = fixed(s, b, x0, K)
                    if K == 1:
                        if not np.array_equal(x, b / 4):
                            w.bad.append(("x == b / 4", xchg, np.flatnonzero(x != b / 4)[:8].tolist()))
                        continue
                    if x[~mask].any():
                        w.bad.append(("zero outside the diamonds", f"{xchg} K={K}",
                                      np.flatnonzero((x != 0) & ~mask)[:8].tolist()))
                    x_ld = pp.reference(m, "comb", K, mloc)[0]
                    elementwise(w, "x inside", x, x_ld, pp.bar(m, K), where=mask, note=f"{xchg} K={K}")
    assert not w.bad, w.bad


# ---- every plan ---------------------------------------------------------------------------------------------
# blocks=3 and blocks=8 give each block several work items (the LDS edge buffer's parity carried from item to item,
# the band walk); blocks=3 also turns the XCD bands off (grid < 8)
RB_PLANS = [f"rb={rb},blocks=8" for rb in (1, 2, 4, 8)]
OTHER_PLANS = ([f"rows={v}" for v in (1, 3, 8, 16)] + [f"bands={v}" for v in (0, 1, 3)] +
               [f"reverse={v}" for v in (0, 1)] + [f"blocks={v}" for v in (3, 8, 64)] + [f"pipe={v}" for v in (0, 1)] +
               ["rows=3,blocks=3,bands=0,reverse=0"] +
               # one-row steps on the occupancy-sized grid (several resident blocks per CU, several steps each): an
               # RB = 1 step puts its edge values into LDS without waiting for its own loads, the closest two steps
               # of one block come to each other (the LDS edge buffer's two halves keep them apart)
               ["rb=1,rows=2", "rb=1,rows=4,bands=0"])
# 130 over two slabs: 9 items of one partial strip per slab, the last of one row; 514: 130 items, the second
# strip one column pair; 1024: full strips, the pipelined catch-up
PLAN_SHAPES = [(130, [0, 0]), (514, None), (1024, None)]


@pytest.mark.parametrize("m,devices", PLAN_SHAPES, ids=[_id(*s) for s in PLAN_SHAPES])
def test_every_plan(monkeypatch, m, devices):
    """Rough data, 9 fixed loops, x every third iteration, under every key of CGX_POISSON_PLAN.  Each plan
    runs twice with equal bits (the last-block sums are deterministic) and agrees with long-double CG element
    by element; with the grid fixed (blocks=8), rb = 1, 2, 4, 8 give x and r.r bit for bit (a thread adds its
    rows in row order whatever RB is: the comment above k_poisson_xr_f64)."""
    K = 9
    b, x0 = pp.rough(m, m)
    x_ld = pp.reference(m, "rough", K)[0]
    bar = pp.bar(m, K)
    runs = {}
    with Worst(f"plans {_id(m, devices)}") as w, solver(monkeypatch, m, devices, "x3") as s:
        for plan in RB_PLANS + OTHER_PLANS:
            monkeypatch.setenv("CGX_POISSON_PLAN", plan)  # read at every launch
            x, rr, _ = fixed(s, b, x0, K)
            x2, rr2, _ = fixed(s, b, x0, K)
            if not (np.array_equal(x, x2) and rr == rr2):
                w.bad.append(("twice", plan, "the second run differs"))
            elementwise(w, "x", x, x_ld, bar, note=plan)
            runs[plan] = (x, rr)
    for plan in RB_PLANS[1:]:
        if not (np.array_equal(runs[plan][0], runs[RB_PLANS[0]][0]) and runs[plan][1] == runs[RB_PLANS[0]][1]):
            w.bad.append(("rb bit for bit", plan, f"differs from {RB_PLANS[0]}"))
    assert not w.bad, w.bad


def test_plans_converge_alike(monkeypatch):
    """b = 1, x0 = 0, eps = 1e-10 on two slabs, as test_poisson_matches_oracle's (130, [0, 0]) case, on the
    grid m = 14: at m = 130 the oracle's sqrt(r.r) is 1.05 eps one loop before its stop and 0.83 eps at it, so a
    loop count there depends on the summation order; m = 14 is the nearest even grid below where the oracle
    alone keeps a factor of 3 on both sides (5.2 and 0.072; _poisson_probe.CONVERGE_M, re-derived by
    test_poisson_probe_cpu.py).  Every plan gives the oracle's loop count and x to TOL."""
    m, eps = pp.CONVERGE_M, pp.CONVERGE_EPS
    xo, K, before, at = pp.stop_margin(m)
    assert before >= pp.MARGIN and at <= 1.0 / pp.MARGIN, (before, at)
    for plan in (None, "rb=1", "rows=3", "blocks=3", "bands=0,reverse=0"):
        with solver(monkeypatch, m, [0, 0], "x3", plan=plan) as s:
            s.fill(1.0, 0.0)
            x, st = s.solve(None, eps=eps)
        assert st.converged and st.iterations == K, (plan, st.iterations, K)
        assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo), plan
