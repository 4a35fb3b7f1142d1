#!/usr/bin/env python3
"""Float-stored against double-stored CSR values (cgx_set_csr_f32 against cgx_set_csr) on one GPU: the same
matrix -- its values rounded to float, and those floats widened for the double-valued context -- on two contexts
that alternate in the same rounds in one process.  Both compute the same bits; only the bytes per entry differ
(8 against 12), so the byte model of a product goes from 12 nnz + 8 (n + 1) + 24 n to 8 nnz + 8 (n + 1) + 24 n.

The two matrices are tools/spmv_ab.py's, built with numpy from nothing but their sizes:
  poisson  the 5-point matrix of an m x m grid (default m = 4096: 16.8 M rows, mean row length 5)
  banded   n = 2^20 rows, half-bandwidth 32 (65 entries per full row), SPD

Protocol: a settle, then --rounds interleaved rounds.  In each round, for the default T of plan_spmv_csr and its
two neighbours (T / 2 and 2 T where instantiated), policy 2: the float-valued and the double-valued context run
--iters fixed-count plain iterations each after one warm iteration, then the same pair with CGX_PC_JACOBI; the
order of the pair is swapped every other round.  Then, per K in --widths, a pair of cgx_create_csr_nrhs contexts
under their default plan in rounds of their own.  The product is timed by the contexts' CGX_TIMING events, the
iteration by the host clock around a synchronize.  One JSON line per round, then summary lines with the medians,
the round-to-round spread ((max - min) / median), the measured double / float ratio, the byte model's ratio and the
share of it reached, (ratio - 1) / (model - 1).

  python tools/csr_f32_ab.py --matrix banded [--logn 20] [--hb 32] [--rounds 5] [--iters 20] [--out profiles/csr_f32_ab_banded.jsonl]
  python tools/csr_f32_ab.py --matrix poisson [--m 4096]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conjugate_gradient_amd as cg  # noqa: E402
from spmv_ab import TS, banded_csr, poisson_csr, time_plan  # noqa: E402

WIDTHS = (2, 4, 8)
KINDS = ("f32", "f64")


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
    ap.add_argument("--widths", type=int, nargs="*", default=list(WIDTHS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join("profiles", f"csr_f32_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    if args.matrix == "poisson":
        indptr, indices, data = poisson_csr(args.m)
        label = f"poisson m={args.m}"
    else:
        indptr, indices, data = banded_csr(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    n, nnz = indptr.size - 1, int(indptr[-1])
    data32 = data.astype(np.float32)
    wide = data32.astype(np.float64)  # what the float-valued context computes with
    del data

    def abytes(kind, K=1):
        return (8 if kind == "f32" else 12) * nnz + 8 * (n + 1) + 24 * K * n

    def model(K=1):
        return abytes("f64", K) / abytes("f32", K)

    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    flags = cg.CGX_F64 | cg.CGX_TIMING

    def make(kind, **kw):
        if kind == "f32":
            s = cg.Solver.from_csr(indptr, indices, data32, flags=flags, a_f32=True, **kw)
            assert s.info.flags & cg.CGX_A_F32
        else:
            s = cg.Solver.from_csr(indptr, indices, wide, flags=flags, **kw)
        return s

    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        def compare(ms, it, K=1):
            """The summary of one configuration: ms[kind] and it[kind] hold one value per round."""
            med = {k: statistics.median(ms[k]) for k in KINDS}
            imed = {k: statistics.median(it[k]) for k in KINDS}
            ratio, iratio = med["f64"] / med["f32"], imed["f64"] / imed["f32"]
            return {"launch_ms": {k: r5(med[k]) for k in KINDS}, "launch_spread": {k: r5(spread(ms[k])) for k in KINDS},
                    "launch_tbs": {k: r5(abytes(k, K) / (med[k] * 1e-3) / 1e12) for k in KINDS},
                    "iteration_ms": {k: r5(imed[k]) for k in KINDS},
                    "iteration_spread": {k: r5(spread(it[k])) for k in KINDS},
                    "launch_ratio": r5(ratio), "iteration_ratio": r5(iratio), "byte_model_ratio": r5(model(K)),
                    "share_of_model": r5((ratio - 1.0) / (model(K) - 1.0)),
                    "faster_beyond_spread": bool(ratio - 1.0 > max(spread(ms[k]) for k in KINDS))}

        # ---- one system: plain and Jacobi, the default T and its neighbours ---------------------------------------
        ctx = {(kind, pc): make(kind, precond=pc) for pc in (None, "jacobi") for kind in KINDS}
        plans = {k: s.matvec_plan() for k, s in ctx.items()}
        T0 = 64 // plans["f32", None]["R"]
        assert all(64 // p["R"] == T0 and p["nt"] == 2 for p in plans.values())  # one default rule for both types
        ts = [T for T in (T0 // 2, T0, 2 * T0) if T in TS]
        emit({"record": "setup", "matrix": label, "n": n, "nnz": nnz, "rounds": args.rounds, "iters": args.iters,
              "default_T": T0, "T": ts, "blocks": {f"{k[0]},{k[1] or 'plain'}": p["blocks"] for k, p in plans.items()},
              "algorithmic_bytes": {k: abytes(k) for k in KINDS}, "byte_model_ratio": r5(model())})
        configs = [(T, pc) for T in ts for pc in (None, "jacobi")]
        t_end = time.perf_counter() + args.settle  # clocks up, code objects loaded, every plan launched once
        while True:
            for T, pc in configs:
                for kind in KINDS:
                    time_plan(ctx[kind, pc], (T, 2), 2)
            if time.perf_counter() >= t_end:
                break
        ms = {c: {k: [] for k in KINDS} for c in configs}
        it = {c: {k: [] for k in KINDS} for c in configs}
        for r in range(args.rounds):
            rec = {}
            for T, pc in configs:
                for kind in (KINDS if r % 2 == 0 else KINDS[::-1]):
                    m, t = time_plan(ctx[kind, pc], (T, 2), args.iters)
                    ms[T, pc][kind].append(m)
                    it[T, pc][kind].append(t)
                rec[f"T={T},{pc or 'plain'}"] = {k: [r5(ms[T, pc][k][r]), r5(it[T, pc][k][r])] for k in KINDS}
            emit({"record": "round", "K": 1, "round": r, "launch_ms,iteration_ms": rec})
        for T, pc in configs:
            emit({"record": "summary", "matrix": label, "K": 1, "T": T, "default_T": T == T0, "precond": pc or "none",
                  **compare(ms[T, pc], it[T, pc])})
        for s in ctx.values():
            s.close()

        # ---- several right-hand sides: the default plan of each width ---------------------------------------------
        for K in args.widths:
            pair = {kind: make(kind, nrhs=K) for kind in KINDS}
            pl = {k: s.matvec_plan() for k, s in pair.items()}
            assert pl["f32"]["R"] == pl["f64"]["R"] and pl["f32"]["nt"] == pl["f64"]["nt"]
            for _ in range(2):
                for kind in KINDS:
                    time_plan(pair[kind], None, 2)
            msk = {k: [] for k in KINDS}
            itk = {k: [] for k in KINDS}
            for r in range(args.rounds):
                for kind in (KINDS if r % 2 == 0 else KINDS[::-1]):
                    m, t = time_plan(pair[kind], None, args.iters)
                    msk[kind].append(m)
                    itk[kind].append(t)
                emit({"record": "round", "K": K, "round": r,
                      "launch_ms,iteration_ms": {k: [r5(msk[k][r]), r5(itk[k][r])] for k in KINDS}})
            emit({"record": "summary", "matrix": label, "K": K, "T": 64 // pl["f32"]["R"],
                  "blocks": {k: pl[k]["blocks"] for k in KINDS}, **compare(msk, itk, K)})
            for s in pair.values():
                s.close()


if __name__ == "__main__":
    main()
