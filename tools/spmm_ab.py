#!/usr/bin/env python3
"""Sweep every instantiated plan (T lanes per row, load policy) of the several-right-hand-sides CSR kernel
k_csr_mult_f64 at K = 2, 4, 8 on one GPU, against the one-system cgx_create_csr context under its default plan,
interleaved in the same rounds in one process.

The two matrices are tools/spmv_ab.py's, built with numpy from nothing but their sizes:
  poisson  the 5-point matrix of an m x m grid (default m = 4096: 16.8 M rows, mean row length 5)
  banded   n = 2^20 rows, half-bandwidth 32 (65 entries per full row), SPD

Protocol, per K: a settle, then --rounds interleaved rounds; in each round every (T, policy) of the K-system
context, the K-system context's default plan and the one-system context's default plan run once, --iters
fixed-count iterations each after one warm iteration (order reversed every other round).  The product is timed
by the contexts' CGX_TIMING events, the iteration by the host clock around a synchronize.  One JSON line per
K and round (ms per launch and per iteration of every configuration), then one summary line per K with the
medians, the round-to-round spread
((max - min) / median), TB/s on the algorithmic bytes 12 nnz + 8 (n + 1) + 24 K n (one system: K = 1), the
system-iterations per second of the K-system context against K one-system iterations, and the byte model's
prediction for that ratio.

  python tools/spmm_ab.py --matrix banded [--logn 20] [--hb 32] [--rounds 5] [--iters 20] [--out profiles/spmm_ab_banded.jsonl]
  python tools/spmm_ab.py --matrix poisson [--m 4096]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conjugate_gradient_amd as cg  # noqa: E402
from spmv_ab import POLICIES, TS, banded_csr, poisson_csr, time_plan  # noqa: E402

WIDTHS = (2, 4, 8)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def r5(v):
    return round(v, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("poisson", "banded"), required=True)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--logn", type=int, default=20)
    ap.add_argument("--hb", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--widths", type=int, nargs="+", default=list(WIDTHS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join("profiles", f"spmm_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    if args.matrix == "poisson":
        indptr, indices, data = poisson_csr(args.m)
        label = f"poisson m={args.m}"
    else:
        indptr, indices, data = banded_csr(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    n, nnz = indptr.size - 1, int(indptr[-1])

    def abytes(K):
        return 12 * nnz + 8 * (n + 1) + 24 * K * n

    def tbs(ms, K):
        return abytes(K) / (ms * 1e-3) / 1e12

    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    flags = cg.CGX_F64 | cg.CGX_TIMING
    one = cg.Solver.from_csr(indptr, indices, data, flags=flags)
    one_plan = one.matvec_plan()
    configs = [(T, nt) for T in TS for nt in POLICIES]
    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        emit({"record": "setup", "matrix": label, "n": n, "nnz": nnz, "rounds": args.rounds, "iters": args.iters,
              "one_system_plan": {"T": 64 // one_plan["R"], "nt": one_plan["nt"], "blocks": one_plan["blocks"]},
              "algorithmic_bytes": {str(K): abytes(K) for K in (1, *args.widths)}})
        for K in args.widths:
            s = cg.Solver.from_csr(indptr, indices, data, nrhs=K, flags=flags)
            d = s.matvec_plan()
            default = (64 // d["R"], d["nt"])
            t_end = time.perf_counter() + args.settle  # clocks up, code objects loaded, every plan launched once
            while True:
                for c in configs:
                    time_plan(s, c, 2)
                time_plan(one, None, 2)
                if time.perf_counter() >= t_end:
                    break
            names = {c: f"T={c[0]},nt={c[1]}" for c in configs}
            names["default"], names["one"] = "default", "one_system_default"
            ms = {c: [] for c in names}
            it = {c: [] for c in names}
            for r in range(args.rounds):
                for c in (configs if r % 2 == 0 else configs[::-1]) + ["default", "one"]:
                    m, t = time_plan(one, None, args.iters) if c == "one" else \
                        time_plan(s, default if c == "default" else c, args.iters)
                    ms[c].append(m)
                    it[c].append(t)
                emit({"record": "round", "K": K, "round": r, "ms": {names[c]: r5(ms[c][r]) for c in names},
                      "iteration_ms": {names[c]: r5(it[c][r]) for c in names}})

            def summ(key, width):
                med = statistics.median(ms[key])
                return {"median_ms": r5(med), "spread": r5(spread(ms[key])), "median_tbs": r5(tbs(med, width)),
                        "iteration_ms_median": r5(statistics.median(it[key])), "iteration_spread": r5(spread(it[key]))}

            best = min(configs, key=lambda c: statistics.median(ms[c]))
            one_it, k_it = statistics.median(it["one"]), statistics.median(it["default"])
            emit({"record": "summary", "matrix": label, "K": K,
                  "plans": {names[c]: summ(c, K) for c in configs},
                  "default_plan": names[default], "default": summ("default", K),
                  "one_system_default": summ("one", 1), "best_plan": names[best],
                  # the K-system iteration against K one-system iterations, both under their default plans
                  "k_iteration_ms": r5(k_it), "k_one_system_iterations_ms": r5(K * one_it),
                  "spread_ms": r5(max(spread(it["default"]) * k_it, K * spread(it["one"]) * one_it)),
                  "system_iterations_per_s": r5(1e3 * K / k_it), "one_system_iterations_per_s": r5(1e3 / one_it),
                  "ratio": r5(K * one_it / k_it),
                  "launch_ratio": r5(K * statistics.median(ms["one"]) / statistics.median(ms["default"])),
                  "byte_model_ratio": r5(K * abytes(1) / abytes(K))})
            s.close()
    one.close()


if __name__ == "__main__":
    main()
