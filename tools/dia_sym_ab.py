#!/usr/bin/env python3
"""The one-sided diagonal SpMV of a symmetric A (k_dia_sym_mult_f64, csrc/cgx_dia_sym.hip) against the full diagonal
SpMV (k_dia_mult_f64) and the CSR SpMV on the same matrix, on one GPU, in interleaved rounds in one process.

Three families:
  sym  cgx_spmv_dia_sym under CGX_DIA_SYM_PLAN, every (R rows per lane, U stored diagonals in flight, load policy of
       the values' last use)
  dia  cgx_spmv_dia under CGX_DIA_PLAN, every (R, U, policy): its best plan is the comparison
  csr  cgx_spmv_csr at the two plans that are its best on these matrices (T = 4 and T = 16, policy 2)
All are kernel-level launches on the null stream, timed alike by one pair of HIP events around --iters launches after
one warm launch.  The matrices are tools/dia_ab.py's: the 5-point Poisson matrix (m = 4096) and the banded one
(n = 2^20, 65 diagonals); the one-sided arrays are their diagonals of offset >= 0.

--iteration: also the time of a fixed-count CG iteration of a one-sided, a diagonal-valued and a CSR context, plain
and with Jacobi, each at its default plan, in the same rounds.

One JSON line per round and configuration, then a summary with the medians, the round-to-round spread, the best plan
of each family and the ratio dia / sym beside the byte model's.  GB/s are on the algorithmic bytes: 8 ndiag_stored n +
16 n for the one-sided kernel, 8 ndiag n + 16 n for DIA, 12 nnz + 8 (n + 1) + 16 n for CSR.

  python tools/dia_sym_ab.py --matrix poisson [--m 4096] [--rounds 5] [--iters 10] [--iteration] [--out FILE]
  python tools/dia_sym_ab.py --matrix banded [--logn 20] [--hb 32]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conjugate_gradient_amd as cg  # noqa: E402
from dia_ab import POLICIES, RS, US, Events, banded_dia, poisson_dia, time_iteration, to_csr  # noqa: E402

CSR_PLANS = ((4, 2), (16, 2))
FAMILIES = ("sym", "dia", "csr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("poisson", "banded"), required=True)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--logn", type=int, default=20)
    ap.add_argument("--hb", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--iteration", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join("profiles", f"dia_sym_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    t0 = time.perf_counter()
    if args.matrix == "poisson":
        offsets, data = poisson_dia(args.m)
        label = f"5-point Poisson m={args.m}"
    else:
        offsets, data = banded_dia(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    n, ndiag = data.shape[1], int(offsets.size)
    up = offsets >= 0
    s_offsets, s_data = np.ascontiguousarray(offsets[up]), np.ascontiguousarray(data[up])
    nstored = int(s_offsets.size)
    for k, o in enumerate(offsets):  # symmetric: diagonal -o is diagonal +o, slot for slot
        if o > 0:
            km = int(np.flatnonzero(offsets == -o)[0])
            assert np.array_equal(data[km, :n - o], data[k, o:]), o
    rp, ci, va = to_csr(offsets, data, n)
    nnz = int(ci.size)
    nbytes = {"sym": 8 * nstored * n + 16 * n, "dia": 8 * ndiag * n + 16 * n, "csr": 12 * nnz + 8 * (n + 1) + 16 * n}
    build_s = time.perf_counter() - t0
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    L, ev = cg.lib(), Events()

    DA = cg.DeviceArray
    d_off, d_data = DA.from_host(offsets), DA.from_host(data.reshape(-1))
    d_soff, d_sdata = DA.from_host(s_offsets), DA.from_host(s_data.reshape(-1))
    d_rp, d_ci, d_va = DA.from_host(rp), DA.from_host(ci), DA.from_host(va)
    v = np.random.default_rng(2).standard_normal(n)
    d_v, d_out = DA.from_host(v), DA(n)

    def launch(family, a, b, nt):
        if family == "sym":
            os.environ["CGX_DIA_SYM_PLAN"] = f"R={a},U={b},nt={nt}"
            rc = L.cgx_spmv_dia_sym(n, nstored, d_soff.ptr, d_sdata.ptr, n, d_v.ptr, d_out.ptr, None)
        elif family == "dia":
            os.environ["CGX_DIA_PLAN"] = f"R={a},U={b},nt={nt}"
            rc = L.cgx_spmv_dia(n, ndiag, d_off.ptr, d_data.ptr, n, d_v.ptr, d_out.ptr, None)
        else:
            os.environ["CGX_SPMV_PLAN"] = f"T={a},nt={nt}"
            rc = L.cgx_spmv_csr(n, n, d_rp.ptr, d_ci.ptr, d_va.ptr, d_v.ptr, d_out.ptr, None)
        assert rc == 0, (family, a, b, nt, rc, L.cgx_last_error())

    def timed(c, iters):
        launch(*c)  # warm
        ev.start()
        for _ in range(iters):
            launch(*c)
        ms = ev.stop()
        assert ms > 0
        return ms / iters

    # the families compute the same product (sym and dia: terms in another order where the offsets are sorted;
    # checked once at the timed size)
    outs = {}
    for c in (("sym", 2, 4, 2), ("dia", 2, 4, 2), ("csr", 4, 0, 2)):
        launch(*c)
        assert L.cgx_dev_synchronize() == 0
        outs[c[0]] = d_out.to_host()
    check = max(float(np.max(np.abs(outs[f] - outs["csr"])) / np.max(np.abs(outs["csr"]))) for f in ("sym", "dia"))
    assert check <= 1e-12, check

    ctxs = {}
    if args.iteration:
        for name in ("CGX_DIA_SYM_PLAN", "CGX_DIA_PLAN", "CGX_SPMV_PLAN"):  # the contexts run their default plans
            os.environ.pop(name, None)
        for name, make in (("sym", lambda p: cg.Solver.from_dia_sym(s_offsets, s_data, precond=p)),
                           ("dia", lambda p: cg.Solver.from_dia(offsets, data, precond=p)),
                           ("csr", lambda p: cg.Solver.from_csr(rp, ci, va, precond=p))):
            for pname, p in (("plain", None), ("jacobi", "jacobi")):
                ctxs[f"{name}_{pname}"] = make(p)

    configs = [(fam, R, U, nt) for fam in ("sym", "dia") for R in RS for U in US for nt in POLICIES] + \
              [("csr", T, 0, nt) for T, nt in CSR_PLANS]
    key = lambda c: f"T={c[1]},nt={c[3]}" if c[0] == "csr" else f"R={c[1]},U={c[2]},nt={c[3]}"  # noqa: E731
    t_end = time.perf_counter() + args.settle  # settle: clocks up, code objects loaded, every plan launched once
    while time.perf_counter() < t_end:
        for c in configs:
            timed(c, 1)
    ms = {c: [] for c in configs}
    it_ms = {k: [] for k in ctxs}
    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        model = nbytes["dia"] / nbytes["sym"]
        emit({"record": "setup", "matrix": label, "n": n, "ndiag": ndiag, "ndiag_stored": nstored, "nnz": nnz,
              "bytes": nbytes, "byte_model_ratio": model, "build_s": round(build_s, 2), "max_rel_diff_vs_csr": check,
              "rounds": args.rounds, "iters": args.iters,
              "default_plans": {k: s.matvec_plan() for k, s in ctxs.items()}})
        for r in range(args.rounds):
            for c in (configs if r % 2 == 0 else configs[::-1]):
                m = timed(c, args.iters)
                ms[c].append(m)
                emit({"record": "round", "round": r, "family": c[0], "plan": key(c), "ms": m,
                      "gbs": nbytes[c[0]] / (m * 1e-3) / 1e9})
            for k, s in ctxs.items():
                m = time_iteration(s, 5 * args.iters)
                it_ms[k].append(m)
                emit({"record": "round", "round": r, "context": k, "iteration_ms": m})

        med = {c: statistics.median(t) for c, t in ms.items()}
        best = {fam: min((c for c in configs if c[0] == fam), key=med.get) for fam in FAMILIES}
        summary = {"record": "summary", "matrix": label,
                   "median_ms": {fam: {key(c): med[c] for c in configs if c[0] == fam} for fam in FAMILIES},
                   "spread": {fam: max((max(ms[c]) - min(ms[c])) / med[c] for c in configs if c[0] == fam)
                              for fam in FAMILIES},
                   "best": {fam: {"plan": key(best[fam]), "ms": med[best[fam]],
                                  "gbs": nbytes[fam] / (med[best[fam]] * 1e-3) / 1e9} for fam in FAMILIES},
                   "dia_over_sym": med[best["dia"]] / med[best["sym"]], "byte_model_ratio": model,
                   "csr_over_sym": med[best["csr"]] / med[best["sym"]]}
        if ctxs:
            summary["iteration_ms_median"] = {k: statistics.median(t) for k, t in it_ms.items()}
            summary["iteration_spread"] = {k: (max(t) - min(t)) / statistics.median(t) for k, t in it_ms.items()}
        emit(summary)
    for s in ctxs.values():
        s.close()


if __name__ == "__main__":
    main()
