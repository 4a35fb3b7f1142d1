#!/usr/bin/env python3
"""Iteration-level A/B of cgx_create_nrhs: one system per pass over A (a plain
cgx_create context, the baseline) against K = 2, 4, 8 systems per pass, all in
one process on one GPU, in interleaved rounds, fixed-count iterations.

Per round and K: ms per iteration (wall clock around `--iters` iterations
bracketed by synchronize, no event packets on the stream), system-iterations
per second (K / time), and the ratio t_K / (K t_1) -- what K systems cost
against K runs of one.  The matVec's own time comes from a second pass with
CGX_TIMING contexts (HIP events around every matVec launch), so the events do
not sit in the iteration timing: ms per launch and TB/s on A's bytes.

One JSON line per round, then one summary line (medians and the spread over
the rounds: (max - min) / median).

  python tools/nrhs_ab.py [--n 65536] [--rounds 5] [--iters 20] [--ks 2,4,8] [--settle 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conjugate_gradient_amd as cg  # noqa: E402


def make(n, k, flags):
    s = cg.Solver(n, flags=flags) if k == 1 else cg.Solver(n, flags=flags, nrhs=k)
    s.generate_spd(42)
    s.begin()
    return s


def restart(s):
    """A fresh solve on the same system: long fixed-count runs would otherwise sink into the subnormals."""
    s.set_x(s.get_x() * 0.0)
    s.begin()


def wall_ms(s, warm, iters):
    restart(s)
    s.iterate(warm, eps=-1.0)
    s.synchronize()
    t0 = time.perf_counter()
    s.iterate(iters, eps=-1.0)
    s.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def matvec_ms(s, warm, iters):
    restart(s)
    s.iterate(warm, eps=-1.0)
    s.reset_timing()
    s.iterate(iters, eps=-1.0)
    st = s.stats()
    return st.matvec_ms / st.matvec_count


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--settle", type=float, default=3.0, help="seconds to idle after the set-up (bench.py's settle)")
    args = ap.parse_args()
    n = args.n
    ks = [1] + [int(v) for v in args.ks.split(",")]
    abytes = 8.0 * n * n

    def phase(flags, fn):
        ctx = {k: make(n, k, flags) for k in ks}
        plans = {k: s.matvec_plan() for k, s in ctx.items()}
        time.sleep(args.settle)
        out = [{k: fn(ctx[k], args.warm, args.iters) for k in ks} for _ in range(args.rounds)]
        for s in ctx.values():
            s.close()
        return out, plans

    it, plans = phase(cg.CGX_F64, wall_ms)
    mv, _ = phase(cg.CGX_F64 | cg.CGX_TIMING, matvec_ms)
    for r in range(args.rounds):
        row = {"n": n, "round": r, "iters": args.iters}
        for k in ks:
            row[f"k{k}"] = {"ms_per_iteration": it[r][k], "system_iterations_per_s": k / it[r][k] * 1e3,
                            "ratio_tk_over_k_t1": it[r][k] / (k * it[r][1]), "matvec_ms": mv[r][k],
                            "matvec_a_tbps": abytes / mv[r][k] / 1e9}
        print(json.dumps(row), flush=True)
    summ = {"n": n, "summary": True, "rounds": args.rounds, "iters": args.iters, "plans": {f"k{k}": plans[k] for k in ks}}
    for k in ks:
        t = [it[r][k] for r in range(args.rounds)]
        m = [mv[r][k] for r in range(args.rounds)]
        ratio = [it[r][k] / (k * it[r][1]) for r in range(args.rounds)]
        summ[f"k{k}"] = {"ms_per_iteration_med": statistics.median(t), "ms_per_iteration_spread": spread(t),
                         "system_iterations_per_s_med": k / statistics.median(t) * 1e3,
                         "ratio_med": statistics.median(ratio), "ratio_spread": spread(ratio),
                         "matvec_ms_med": statistics.median(m), "matvec_ms_spread": spread(m),
                         "matvec_a_tbps_med": abytes / statistics.median(m) / 1e9}
    print(json.dumps(summ), flush=True)


if __name__ == "__main__":
    main()
