"""fp64 CG beyond five live iterations, through every iteration form.

The systems are tests/_long_systems.py's: the loop stops at a sharp K >= 13 (18 at m = 16), x0 is nonzero, and
a fixed count of F = m + 10 keeps r.r live (about 1e-31, not underflowed), so the state indexed by the
iteration number -- the scalar rings of 4, the event ring of 8, the fold's p buffer by the parity of k -- is
carried through several laps with live values.

Bars (S = _long_systems.long_system(n); every reference quantity is numpy's, none is the code under test):
  loop count   with eps = S["eps"]: iterations == K and converged == 1
  at the stop  ||b - A x|| <= eps (the stopping rule's own bound) and ||x - x_direct|| <= 1.01 eps
               (||A^-1|| = 1 / lambda_min = 1)
  fixed count  rel(x, X[F]) <= 1e-12, the suite's bar for fixed-count agreement (the three summation orders
               agree to 5e-14 there; test_long_systems_cpu asserts 1e-13)
  history      begin(), iterate(1) up to k = m - 4: sqrt(stats().rr) within T_h of h[k]; x at k = m - 8 within
               T_x; T_h, T_x = 100 x the measured spread of the three orders (caps 1e-8 / 1e-10 asserted on the CPU)
Where the project claims bit equality between forms, it is asserted here as well, on x after every iterate(3)
piece from begin() to K, on the loop count and on r.r.

Each test prints its worst measured ratio to each bar (pytest -s).
"""
import numpy as np
import pytest

import _long_systems as ls
import conjugate_gradient_amd as cg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    assert cg.device_count() >= 1, "no GPU visible: the HIP path must run"


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Worst:
    """The worst measured ratio to each bar within one test, printed at its end."""

    def __init__(self, what):
        self.what, self.r = what, {}

    def ratio(self, bar, value, bound):
        self.r[bar] = max(self.r.get(bar, 0.0), float(value) / float(bound))
        return value <= bound

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        print(f"\n[long] {self.what}: " + ", ".join(f"{k} {v:.3g}" for k, v in self.r.items()))


def run_all(s, S, eps=None):
    """On context s with S set: the solve to eps, the same solve in iterate(3) pieces (x after every piece),
    and the fixed count F."""
    eps = S["eps"] if eps is None else eps
    before = s.stats().total_iterations  # counted over the context's life
    x, st = s.solve(S["x0"], eps=eps)
    out = dict(x=x, it=st.iterations, conv=st.converged, rr=st.rr, total=s.stats().total_iterations - before)
    s.set_x(S["x0"])
    s.begin()
    xs, total = [], 0
    while True:
        d, conv = s.iterate(3, eps=eps)
        total += d
        xs.append(s.get_x())
        if conv or d == 0:
            break
        assert total <= 2 * S["K"], "the solve in pieces does not stop"
    out.update(pieces=xs, pit=total, prr=s.stats().rr)
    xF, stF = s.solve(S["x0"], eps=-1.0, max_iter=S["F"])
    out.update(xF=xF, itF=stF.iterations, rrF=stF.rr)
    return out


def meets_bars(w, S, r, key=""):
    A, b, K, eps = S["A"], S["b"], S["K"], S["eps"]
    assert r["it"] == K and r["conv"] == 1 and r["total"] == K, (key, r["it"], K)
    assert r["pit"] == K and len(r["pieces"]) == (K + 2) // 3, (key, r["pit"])
    assert w.ratio("sqrt(rr)/eps", np.sqrt(r["rr"]), eps) and r["prr"] == r["rr"], key
    assert np.array_equal(r["pieces"][-1], r["x"]), key
    assert w.ratio("residual/eps", np.linalg.norm(b - A @ r["x"]), eps), key
    assert w.ratio("error/(1.01 eps)", np.linalg.norm(r["x"] - S["x_direct"]), 1.01 * eps), key
    assert r["itF"] == S["F"] and np.isfinite(r["rrF"]) and r["rrF"] > 0.0, key
    assert w.ratio("x_F/1e-12", rel(r["xF"], S["X"][S["F"]]), 1e-12), key


def same_run(a, b):
    return (a["it"] == b["it"] and a["rr"] == b["rr"] and np.array_equal(a["x"], b["x"])
            and len(a["pieces"]) == len(b["pieces"]) and all(np.array_equal(p, q) for p, q in zip(a["pieces"], b["pieces"]))
            and np.array_equal(a["xF"], b["xF"]) and a["rrF"] == b["rrF"])


def follows_history(w, s, S, key=""):
    m, h, X = S["m"], S["h"], S["X"]
    s.set_x(S["x0"])
    s.begin()
    for k in range(1, m - 4 + 1):
        d, _ = s.iterate(1)
        assert d == 1
        got = np.sqrt(s.stats().rr)
        assert w.ratio("history/T_h", abs(got - h[k]) / h[k], S["T_h"]), (key, k, got, h[k])
        if k == m - 8:
            assert w.ratio("x(m-8)/T_x", rel(s.get_x(), X[k]), S["T_x"]), (key, k)


# ---- one GPU, dense ---------------------------------------------------------------------------
FORMS = (("three", "0", "0"), ("two", "1", "0"), ("fold", "1", "1"))


@pytest.mark.parametrize("n", [130, 1001, 4096])
def test_one_gpu_every_form(monkeypatch, n):
    """Three launches / two / folded x device-gated (CGX_LOOKAHEAD 1, 2, 5, 7) / host-checked: every
    combination meets the bars and all agree bit for bit -- x after every piece, loop count, r.r
    (test_two_launch_iteration_bitwise_equals_three and test_device_gated_convergence_matches_host_checked
    claim it on solves of at most 5 iterations).  n = 4096 is CGX_SMALL_ACTIVE with two blocks in
    k_update_xrp_f64; there CGX_MV_SMALL=0 agrees to 1e-12 at F."""
    S = ls.long_system(n)
    res = {}
    with Worst(f"one GPU n={n} K={S['K']} F={S['F']}") as w:
        for form, fuse, fold in FORMS:
            monkeypatch.setenv("CGX_FUSE_P", fuse)
            monkeypatch.setenv("CGX_FOLD_P", fold)
            with cg.Solver(n) as s:
                assert bool(s.info.flags & cg.CGX_FUSED_ACTIVE) == (fuse == "1")
                assert bool(s.info.flags & cg.CGX_FOLD_ACTIVE) == (fold == "1")
                assert bool(s.info.flags & cg.CGX_SMALL_ACTIVE) == (n == 4096)
                s.set_system(S["A"], S["b"], S["x0"])
                for gated, look in (("0", "1"), ("1", "1"), ("1", "2"), ("1", "5"), ("1", "7")):
                    monkeypatch.setenv("CGX_GATED", gated)
                    monkeypatch.setenv("CGX_LOOKAHEAD", look)
                    res[(form, gated, look)] = r = run_all(s, S)
                    meets_bars(w, S, r, (form, gated, look))
                follows_history(w, s, S, form)
        ref = res[("three", "0", "1")]
        for key, r in res.items():
            assert same_run(r, ref), key
        if n == 4096:
            monkeypatch.setenv("CGX_MV_SMALL", "0")
            with cg.Solver(n) as s:
                assert not s.info.flags & cg.CGX_SMALL_ACTIVE
                s.set_system(S["A"], S["b"], S["x0"])
                r = run_all(s, S)
                meets_bars(w, S, r, "CGX_MV_SMALL=0")
            assert w.ratio("small vs L2 at F/1e-12", rel(r["xF"], ref["xF"]), 1e-12)


@pytest.mark.parametrize("n", [130, 1001])
def test_matvec_plan_switched_mid_solve(n):
    """The matVec plan changed between the iterate(3) pieces of one solve.  Chunks in flight and load policy
    (the plans of test_matvec_f64_every_plan_bitwise_equal with the context's rows per wave and grid) leave
    every row sum and the order of the fused p.Ap as they are: x stays bit-identical to the unswitched
    solve after every piece -- with the fold active, which these plans keep.  Other rows per wave give another
    grid, so another order of the p.Ap partials: on the three-launch form those are switched too and the
    solve still stops at K and meets the bars."""
    S = ls.long_system(n)
    K, eps = S["K"], S["eps"]
    with Worst(f"plan switches n={n}") as w, cg.Solver(n) as s:
        assert s.info.flags & cg.CGX_FOLD_ACTIVE
        s.set_system(S["A"], S["b"], S["x0"])
        base = run_all(s, S)
        meets_bars(w, S, base, "unswitched")
        p0 = s.matvec_plan()
        plans = []
        for U in (2, 4, 8):
            for nt in (0, 1, 2, 8):
                if not (p0["R"] == 8 and U == 8 and nt in (2, 8)):
                    s.set_matvec_plan(p0["R"], U, nt)
                    if s.matvec_plan()["blocks"] == p0["blocks"]:
                        plans.append((p0["R"], U, nt))
        assert len(plans) >= 6, (p0, plans)
        for start in (0, 5):
            s.set_matvec_plan(*plans[start])
            s.set_x(S["x0"])
            s.begin()
            total = 0
            for i, want in enumerate(base["pieces"]):
                d, conv = s.iterate(3, eps=eps)
                total += d
                assert s.info.flags & cg.CGX_FOLD_ACTIVE
                assert np.array_equal(s.get_x(), want), (start, i, plans[(start + i) % len(plans)])
                s.set_matvec_plan(*plans[(start + i + 1) % len(plans)])
            assert conv and total == K and s.stats().rr == base["rr"]
    with Worst(f"rows per wave switched n={n}") as w, cg.Solver(n) as s:
        s.set_system(S["A"], S["b"], S["x0"])
        s.set_matvec_plan(4, 8)  # turns the fold off for the solves that follow
        assert not s.info.flags & cg.CGX_FOLD_ACTIVE
        s.begin()
        total = 0
        for R, U, nt in ((1, 2, 0), (8, 4, 1), (2, 8, 8), (4, 2, 2), (1, 8, 1), (8, 2, 0), (2, 4, 2)):
            d, conv = s.iterate(3, eps=eps)
            total += d
            if conv:
                break
            s.set_matvec_plan(R, U, nt)
        x, st = s.get_x(), s.stats()
        assert conv and total == K and st.iterations == K
        assert w.ratio("residual/eps", np.linalg.norm(S["b"] - S["A"] @ x), eps)
        assert w.ratio("error/(1.01 eps)", np.linalg.norm(x - S["x_direct"]), 1.01 * eps)


# ---- row blocks in one process ----------------------------------------------------------------
@pytest.mark.parametrize("n,P", [(1000, 8), (2304, 2), (2304, 3)])
def test_row_blocks_every_exchange(monkeypatch, n, P):
    """Row blocks on device 0: 125-row blocks (unaligned slices, the scalar kernels, no overlap) and
    128-aligned ones with the overlapped gather on and off; pull kernels with folded combines, one enqueuing
    thread per block, a combine kernel per scalar, per-pair peer copies.  Bit-equal among themselves
    (test_local_exchange_kernels_bitwise_equal_peer_copies and test_overlap_choice_is_bitwise_neutral claim it
    on short solves), each meets the bars; the forms without folded combines report r.r mid-solve and follow
    the history."""
    S = ls.long_system(n)
    res = {}
    with Worst(f"row blocks n={n} P={P} K={S['K']}") as w:
        for overlap in (("0", "1") if n % (128 * P) == 0 else ("0",)):
            monkeypatch.setenv("CGX_OVERLAP", overlap)
            for form in ("kernel", "threads", "nofuse", "copy"):
                monkeypatch.setenv("CGX_LOCAL_XCHG", "copy" if form == "copy" else "kernel")
                monkeypatch.setenv("CGX_LOCAL_FUSE", "0" if form == "nofuse" else "1")
                monkeypatch.setenv("CGX_LOCAL_THREADS", "1" if form == "threads" else "0")
                with cg.Solver(n, devices=[0] * P) as s:
                    assert s.info.nshards == P
                    assert bool(s.info.flags & cg.CGX_OVERLAP_ACTIVE) == (overlap == "1")
                    s.set_system(S["A"], S["b"], S["x0"])
                    res[(overlap, form)] = r = run_all(s, S)
                    meets_bars(w, S, r, (overlap, form))
                    if not s.info.flags & cg.CGX_FOLDED_ACTIVE:
                        follows_history(w, s, S, (overlap, form))
                    else:
                        assert form in ("kernel", "threads")
        ref = res[("0", "copy")]
        for key, r in res.items():
            assert same_run(r, ref), key


@pytest.mark.parametrize("mode", ["collective", "deterministic"])
def test_rank_mode_world1(mode):
    """One rank of a one-process-per-GPU job at world size 1, plain and CGX_DETERMINISTIC (the rank-order
    combine: the single-shard bits)."""
    S = ls.long_system(1000)
    flags = cg.CGX_F64 | (cg.CGX_DETERMINISTIC if mode == "deterministic" else 0)
    with Worst(f"rank mode {mode} n=1000") as w:
        with cg.Solver(1000, rank=0, nranks=1, unique_id=cg.get_unique_id(), device=0, flags=flags) as s:
            s.set_system(S["A"], S["b"], S["x0"])
            r = run_all(s, S)
            meets_bars(w, S, r, mode)
            follows_history(w, s, S, mode)
        if mode == "deterministic":
            with cg.Solver(1000) as s:
                s.set_system(S["A"], S["b"], S["x0"])
                assert same_run(run_all(s, S), r)


# ---- symmetric tiles and host-streamed A ----------------------------------------------------------
@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("n", [1000, 2304])
def test_symmetric_long(monkeypatch, n, stream):
    """CGX_SYMMETRIC, resident and host-streamed (1 MiB chunks): the bars, the history, and the same x twice
    on one context."""
    monkeypatch.setenv("CGX_STREAM_TILE_MB", "1")
    S = ls.long_system(n)
    flags = cg.CGX_F64 | cg.CGX_SYMMETRIC | (cg.CGX_HOST_STREAM if stream else 0)
    with Worst(f"symmetric{' streamed' if stream else ''} n={n} K={S['K']}") as w, cg.Solver(n, flags=flags) as s:
        s.set_system(S["A"], S["b"], S["x0"])
        r1 = run_all(s, S)
        meets_bars(w, S, r1)
        follows_history(w, s, S)
        assert same_run(run_all(s, S), r1)


@pytest.mark.parametrize("P", [1, 2])
def test_host_streamed_rows_long(monkeypatch, P):
    """CGX_HOST_STREAM row-major, 1 and 2 row blocks, n = 2304."""
    monkeypatch.setenv("CGX_STREAM_TILE_MB", "1")
    S = ls.long_system(2304)
    with Worst(f"host-streamed rows P={P} n=2304") as w:
        with cg.Solver(2304, flags=cg.CGX_F64 | cg.CGX_HOST_STREAM, devices=None if P == 1 else [0] * P) as s:
            s.set_system(S["A"], S["b"], S["x0"])
            r = run_all(s, S)
            meets_bars(w, S, r)
            if not s.info.flags & cg.CGX_FOLDED_ACTIVE:
                follows_history(w, s, S)


# ---- several right-hand sides ---------------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs", [(130, 8), (130, 3), (1000, 8), (1000, 3)])
def test_nrhs_long(monkeypatch, n, nrhs):
    """cgx_create_nrhs: column j is (s_j b, s_j x0), s_j a power of two from _long_systems.column_scales, so one
    common eps stops the columns at K, K + 1 and K + 2.  Per column: the loop count K_j and the bars (against
    s_j x the references); a stopped column's x is the same bits whether its neighbours go on or stop with
    it (test_freeze's claim, here with live iterations after the freeze); permuting the columns permutes the
    results; a fixed count F per column; gated and CGX_GATED=0 the same bits."""
    S = ls.long_system(n)
    A, eps, K, F = S["A"], S["eps"], S["K"], S["F"]
    sc, Ks = ls.column_scales(S, nrhs)
    assert len(set(Ks)) >= 3 and min(Ks) >= 13
    B, X0 = np.stack([v * S["b"] for v in sc]), np.stack([v * S["x0"] for v in sc])
    perm = list(np.random.default_rng(nrhs).permutation(nrhs))
    res = {}
    with Worst(f"nrhs={nrhs} n={n} K_j={Ks}") as w:
        for gated in ("1", "0"):
            monkeypatch.setenv("CGX_GATED", gated)
            with cg.Solver(n, nrhs=nrhs) as s:
                s.set_system(A, B, X0)
                X, st = s.solve(X0, eps=eps)
                per = [s.stats_rhs(j) for j in range(nrhs)]
                s.set_system(A, B[perm], X0[perm])
                XP, _ = s.solve(X0[perm], eps=eps)
                itp = [s.stats_rhs(j).iterations for j in range(nrhs)]
                # every column at scale 1: all stop at K together
                s.set_system(A, np.stack([S["b"]] * nrhs), np.stack([S["x0"]] * nrhs))
                XE, ste = s.solve(np.stack([S["x0"]] * nrhs), eps=eps)
                s.set_system(A, B, X0)
                XF, stf = s.solve(X0, eps=-1.0, max_iter=F)
            its = [p.iterations for p in per]
            assert its == Ks and all(p.converged == 1 for p in per), (gated, its, Ks)
            assert st.iterations == max(Ks) and st.converged == 1
            for j in range(nrhs):
                assert w.ratio("sqrt(rr_j)/eps", np.sqrt(per[j].rr), eps), j
                assert w.ratio("residual/eps", np.linalg.norm(B[j] - A @ X[j]), eps), j
                assert w.ratio("error/(1.01 eps)", np.linalg.norm(X[j] - sc[j] * S["x_direct"]), 1.01 * eps), j
                assert w.ratio("x_F/1e-12", rel(XF[j], sc[j] * S["X"][F]), 1e-12), j
            assert stf.iterations == F
            assert np.array_equal(XP, X[perm]) and itp == [Ks[p] for p in perm], gated
            assert ste.iterations == K and all(np.array_equal(XE[j], XE[0]) for j in range(nrhs))
            early = [j for j in range(nrhs) if Ks[j] == K]  # scale 1: stopped first, the neighbours went on
            assert early and all(sc[j] == 1.0 and np.array_equal(X[j], XE[j]) for j in early), gated
            res[gated] = (X, its, [p.rr for p in per], XF)
        assert np.array_equal(res["1"][0], res["0"][0]) and res["1"][1:3] == res["0"][1:3]
        assert np.array_equal(res["1"][3], res["0"][3])
        with cg.Solver(n) as one:  # the one-system context stops every column at the same K_j
            one.set_system(A, B[0], X0[0])
            for j in range(nrhs):
                one.set_rows(0, None, B[j])
                _, s1 = one.solve(X0[j], eps=eps)
                assert s1.iterations == Ks[j], (j, s1.iterations, Ks[j])


# ---- CGX_A_F32 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ls.A32_SIZES)
def test_a_f32_long(monkeypatch, n):
    """Rounding A to float destroys the clustered spectrum: no cliff, about 45 live iterations, so no loop
    count is checked.  A fixed count of 48 against the numpy history on A32.astype(float64), at 1e-12 (the
    orders agree to 4e-14 there; sqrt(r.r) is 1e-20 .. 1e-14).  Every iteration form of
    test_every_chunk_and_tail_boundary_every_iteration_form -- three launches and two, the fixed-count loop,
    the device-gated and the host-checked one (a stopping test that never fires: eps = 1e-300), and the
    solve in iterate(3) pieces -- gives the same x bit for bit; a CGX_F64 context on the widened matrix meets
    the same bar."""
    A32, Aw, b, x0 = ls.widened_a32(n)
    C = ls.A32_COUNT
    _, X = ls.history(Aw, b, x0, C)
    res = {}
    with Worst(f"CGX_A_F32 n={n} count={C}") as w:
        for fuse in ("0", "1"):
            monkeypatch.setenv("CGX_FUSE_P", fuse)
            for gated in ("1", "0"):
                monkeypatch.setenv("CGX_GATED", gated)
                with cg.Solver(n, flags=cg.CGX_A_F32) as s:
                    assert bool(s.info.flags & cg.CGX_FUSED_ACTIVE) == (fuse == "1")
                    assert not s.info.flags & (cg.CGX_FOLD_ACTIVE | cg.CGX_SMALL_ACTIVE)
                    s.set_system(A32, b, x0)
                    xf, stf = s.solve(x0, eps=-1.0, max_iter=C)
                    xt, stt = s.solve(x0, eps=1e-300, max_iter=C)
                    s.set_x(x0)
                    s.begin()
                    done = sum(s.iterate(3, eps=1e-300)[0] for _ in range(C // 3))
                    xp, rrp = s.get_x(), s.stats().rr
                assert stf.iterations == stt.iterations == done == C and stt.converged == 0
                assert w.ratio("x_48/1e-12", rel(xf, X[C]), 1e-12), (fuse, gated)
                assert np.isfinite(stf.rr) and stf.rr > 0.0  # live ratios to the end
                res[(fuse, gated)] = (xf, stf.rr)
                assert np.array_equal(xt, xf) and np.array_equal(xp, xf) and stt.rr == stf.rr == rrp, (fuse, gated)
        ref = res[("0", "0")]
        for key, (x, rr) in res.items():
            assert np.array_equal(x, ref[0]) and rr == ref[1], key
        monkeypatch.setenv("CGX_FUSE_P", "1")
        with cg.Solver(n) as s:
            s.set_system(Aw, b, x0)
            xw, stw = s.solve(x0, eps=-1.0, max_iter=C)
        assert stw.iterations == C
        assert w.ratio("CGX_F64 on the widened A: x_48/1e-12", rel(xw, X[C]), 1e-12)
