#!/usr/bin/env python3
"""Sweep the fp64 matVec plan (rows per wave R, chunks in flight U, non-temporal
A loads, resident blocks per CU) on one GPU, interleaved rounds in one process
(cdna_hip_programming.md s5.4 rule 24).  Prints one JSON line per config with
the median / min matVec kernel time (HIP events) and algorithmic GB/s.

  python tools/sweep_matvec.py [--n 65536] [--rounds 3] [--iters 4]

--a-fp32: the CGX_A_F32 kernel's plans (float A, fp64 arithmetic) instead, with
the CGX_F64 default plan in the same rounds on the same generated system;
GB/s on the bytes each algorithm needs (4 N^2 + 16 N against 8 N^2 + 16 N).
Then one fixed-count run of 20 iterations per mode, bracketed by synchronize,
for iterations/s, and -- the correctness cross-check at the timed size -- a
solve to 1e-10 under CGX_A_F32 with its true residual.

  python tools/sweep_matvec.py --a-fp32 [--n 65536] [--rounds 5] [--iters 4]

--nrhs K: the instantiated plans of k_matvec_nrhs_f64 (cgx_create_nrhs, K
right-hand sides per pass over A) in the same form: interleaved rounds, the
k_matvec_f64 default plan in the same rounds, every plan's first launch
recorded apart ("record": "first").

  python tools/sweep_matvec.py --nrhs 4 [--n 65536] [--rounds 5] [--iters 4]
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conjugate_gradient_amd as cg  # noqa: E402

A32_PLANS = [(1, 4), (1, 8), (2, 4), (4, 2), (4, 4), (8, 2)]


def time_plan(s, plan, iters):
    """ms per matVec launch (CGX_TIMING events) of `iters` fixed iterations under `plan` (None: as is)."""
    if plan is not None:
        s.set_matvec_plan(*plan)
    s.iterate(1, eps=-1.0)  # warm this plan
    s.reset_timing()
    s.iterate(iters, eps=-1.0)
    st = s.stats()
    return st.matvec_ms / st.matvec_count


def sweep_a32(args):
    n = args.n
    s64 = cg.Solver(n, flags=cg.CGX_F64 | cg.CGX_TIMING)
    s32 = cg.Solver(n, flags=cg.CGX_A_F32 | cg.CGX_TIMING)
    for s in (s64, s32):
        s.generate_spd(42)
        s.begin()
    nts = [int(v) for v in args.nt.split(",")] if args.nt != "0,1" else [2, 8]
    configs = [(R, U, nt, 0) for (R, U) in A32_PLANS for nt in nts]
    times = {c: [] for c in configs}
    times["f64"] = []
    plans = {"f64": s64.matvec_plan()}
    for _ in range(args.rounds):
        times["f64"].append(time_plan(s64, None, args.iters))
        for c in configs:
            times[c].append(time_plan(s32, c, args.iters))
            plans[c] = s32.matvec_plan()
    rows = []
    for c, t in times.items():
        nbytes = (8 if c == "f64" else 4) * n * n + 16 * n
        med, mn, mx = statistics.median(t), min(t), max(t)
        pl = plans[c]
        rows.append({"mode": "CGX_F64" if c == "f64" else "CGX_A_F32", "n": n, "R": pl["R"], "U": pl["U"], "nt": pl["nt"],
                     "blocks": pl["blocks"], "rounds": len(t), "ms_med": med, "ms_min": mn, "ms_max": mx,
                     "bytes": nbytes, "gbps_med": nbytes / med / 1e6, "gbps_best": nbytes / mn / 1e6})
    rows.sort(key=lambda r: r["ms_med"])
    for r in rows:
        print(json.dumps(r), flush=True)
    best = next(r for r in rows if r["mode"] == "CGX_A_F32")
    # iterations/s: 20 fixed iterations per mode (twice, alternating), the A_F32 context on the sweep's best plan
    for name, s, plan in (("CGX_F64", s64, None), ("CGX_A_F32 best", s32, (best["R"], best["U"], best["nt"], 0)),
                          ("CGX_F64", s64, None), ("CGX_A_F32 best", s32, (best["R"], best["U"], best["nt"], 0))):
        if plan is not None:
            s.set_matvec_plan(*plan)
        s.generate_spd(42)
        s.begin()
        s.iterate(3, eps=-1.0)
        s.synchronize()
        t0 = time.perf_counter()
        s.iterate(20, eps=-1.0)
        s.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"mode": name, "n": n, "plan": s.matvec_plan(), "fixed_iterations": 20,
                          "ms_per_iteration": dt / 20 * 1e3, "iterations_per_s": 20 / dt}), flush=True)
    s64.close()
    s32.close()
    # the default plan of a fresh context, and the correctness cross-check at the timed size
    with cg.Solver(n, flags=cg.CGX_A_F32) as s:
        s.generate_spd(42)
        x, st = s.solve(None, eps=1e-10)
        rn, bn = s.residual_norm()
        print(json.dumps({"mode": "CGX_A_F32 default", "n": n, "plan": s.matvec_plan(), "solve_eps": 1e-10,
                          "iterations": st.iterations, "converged": st.converged, "solve_ms": st.solve_ms,
                          "residual_norm": rn, "b_norm": bn, "residual_below_stop": bool(rn < 1e-10 * bn)}), flush=True)


NRHS_PLANS = {2: [(2, 4), (4, 2), (4, 4), (8, 2)], 4: [(4, 2), (4, 4), (8, 2)], 8: [(4, 1), (4, 2)]}


def time_plan_first(s, plan, iters):
    """(ms of the plan's first launch in this process, ms per launch of the `iters` after it)."""
    if plan is not None:
        s.set_matvec_plan(*plan)
    s.reset_timing()
    s.iterate(1, eps=-1.0)
    first = s.stats()
    first_ms = first.matvec_ms / first.matvec_count
    s.reset_timing()
    s.iterate(iters, eps=-1.0)
    st = s.stats()
    return first_ms, st.matvec_ms / st.matvec_count


def sweep_nrhs(args):
    """The instantiated plans of k_matvec_nrhs_f64 for nrhs = K, interleaved with the k_matvec_f64 default plan
    in the same rounds on the same generated A.  GB/s on A's bytes plus the vectors each launch needs
    (8 N^2 + 16 K N against 8 N^2 + 16 N).  Round 0's first launch of every plan goes to records of its own
    ("record": "first"), not into the medians."""
    n, K = args.n, args.nrhs
    width = 2 if K <= 2 else 4 if K <= 4 else 8
    s1 = cg.Solver(n, flags=cg.CGX_F64 | cg.CGX_TIMING)
    sk = cg.Solver(n, flags=cg.CGX_F64 | cg.CGX_TIMING, nrhs=K)
    for s in (s1, sk):
        s.generate_spd(42)
        s.begin()
    nts = [int(v) for v in args.nt.split(",")] if args.nt != "0,1" else [2, 8]
    configs = [(R, U, nt, 0) for (R, U) in NRHS_PLANS[width] for nt in nts]
    times = {c: [] for c in configs}
    times["f64"] = []
    firsts = {}
    plans = {"f64": s1.matvec_plan(), "default": sk.matvec_plan()}
    for rnd in range(args.rounds):
        f, t = time_plan_first(s1, None, args.iters)
        times["f64"].append(t)
        firsts.setdefault("f64", f)
        for c in configs:
            f, t = time_plan_first(sk, c, args.iters)
            times[c].append(t)
            firsts.setdefault(c, f)
            plans[c] = sk.matvec_plan()
    rows = []
    for c, t in times.items():
        k = 1 if c == "f64" else K
        nbytes = 8 * n * n + 16 * k * n
        med, mn, mx = statistics.median(t), min(t), max(t)
        pl = plans[c]
        rows.append({"record": "sweep", "kernel": "k_matvec_f64" if c == "f64" else "k_matvec_nrhs_f64", "n": n,
                     "nrhs": k, "R": pl["R"], "U": pl["U"], "nt": pl["nt"], "blocks": pl["blocks"], "rounds": len(t),
                     "ms_med": med, "ms_min": mn, "ms_max": mx, "bytes": nbytes, "gbps_med": nbytes / med / 1e6,
                     "gbps_best": nbytes / mn / 1e6, "a_tbps_med": 8 * n * n / med / 1e9})
    rows.sort(key=lambda r: r["ms_med"])
    for r in rows:
        print(json.dumps(r), flush=True)
    for c, f in firsts.items():
        pl = plans[c]
        print(json.dumps({"record": "first", "kernel": "k_matvec_f64" if c == "f64" else "k_matvec_nrhs_f64", "n": n,
                          "nrhs": 1 if c == "f64" else K, "R": pl["R"], "U": pl["U"], "nt": pl["nt"], "ms": f}),
              flush=True)
    print(json.dumps({"record": "default_plan", "n": n, "nrhs": K, "plan": plans["default"]}), flush=True)
    s1.close()
    sk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--R", default="1,2,4,8")
    ap.add_argument("--U", default="2,4,8")
    ap.add_argument("--nt", default="0,1")
    ap.add_argument("--bpc", default="0")
    ap.add_argument("--a-fp32", action="store_true", help="the CGX_A_F32 plans beside the CGX_F64 default")
    ap.add_argument("--nrhs", type=int, default=0,
                    help="K: the plans of k_matvec_nrhs_f64 for K right-hand sides beside the k_matvec_f64 default")
    args = ap.parse_args()
    if args.a_fp32:
        return sweep_a32(args)
    if args.nrhs:
        return sweep_nrhs(args)
    n = args.n
    s = cg.Solver(n, flags=cg.CGX_F64 | cg.CGX_TIMING)
    s.generate_spd(42)
    s.begin()
    configs = list(itertools.product(*(map(int, v.split(",")) for v in (args.R, args.U, args.nt, args.bpc))))
    times = {c: [] for c in configs}
    plans = {}
    bytes_launch = 8 * n * n + 16 * n
    for _ in range(args.rounds):
        for c in configs:
            s.set_matvec_plan(*c)
            plans[c] = s.matvec_plan()
            s.iterate(1, eps=-1.0)  # warm this plan
            s.reset_timing()
            s.iterate(args.iters, eps=-1.0)
            st = s.stats()
            times[c].append(st.matvec_ms / st.matvec_count)
    rows = []
    for c in configs:
        med, mn = statistics.median(times[c]), min(times[c])
        rows.append({"R": c[0], "U": c[1], "nt": c[2], "bpc": c[3], "blocks": plans[c]["blocks"],
                     "ms_med": med, "ms_min": mn, "gbps_med": bytes_launch / med / 1e6, "gbps_best": bytes_launch / mn / 1e6})
    rows.sort(key=lambda r: r["ms_med"])
    for r in rows:
        print(json.dumps(r))
    s.close()


if __name__ == "__main__":
    main()
