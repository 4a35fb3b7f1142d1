#!/usr/bin/env python3
"""Jacobi-preconditioned CG against plain CG on a cgx_create_csr context, one GPU, in interleaved rounds in one
process -- what the extra 8-byte stream of the two PCG update kernels (cgx_pcg.hip) costs per iteration, and what
the preconditioner buys end to end.

The matrices are tools/spmv_ab.py's: poisson (5-point, m x m grid, default m = 4096) and banded (n = 2^20,
half-bandwidth 32).

Protocol: a settle, then --rounds interleaved rounds; in each round the plain form and the Jacobi form run --iters
fixed-count iterations each after a warm one, in alternating order.  Per form and round: ms per iteration by the
host clock around a synchronize, ms per SpMV launch by the context's CGX_TIMING events, and their difference -- the
two update kernels with the launch gaps, which is where the forms differ (plain: 24 + 40 B per row, Jacobi: 32 + 48).
One JSON line per round and form, then a summary with the medians, the round-to-round spread ((max - min) / median),
the update kernels' TB/s on those bytes and the one-time extraction (cgx_set_precond(CGX_PC_JACOBI), host clock).

--plain-only: only the plain form (a tree without the feature: --root names the checkout whose package is loaded),
for timing a baseline library in alternating processes with the same tool.
--solve DEC: one end-to-end line on the matrix scaled by DEC decades (A' = D^(1/2) A D^(1/2), d_i = 10 ** (DEC *
((i * 7919) mod n) / n), b' = D^(1/2) 1), eps = 1e-8 ||b'||: loops and wall time of the Jacobi form and of the plain
form, plain capped at --plain-cap loops.

  python tools/pcg_ab.py --matrix banded [--rounds 5] [--iters 50] [--solve 6] [--out profiles/pcg_ab_banded.jsonl]
  python tools/pcg_ab.py --matrix poisson --plain-only --root /path/to/baseline/checkout
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN_B, PCG_B = 24 + 40, 32 + 48  # bytes per row of the two update kernels


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def time_form(s, iters):
    """(ms per iteration, ms per SpMV launch) of `iters` fixed-count iterations of the context as it is set up."""
    s.fill(1.0, 0.0)
    s.begin()
    s.iterate(1, eps=-1.0)
    s.reset_timing()
    s.synchronize()
    t0 = time.perf_counter()
    s.iterate(iters, eps=-1.0)
    s.synchronize()
    dt = time.perf_counter() - t0
    st = s.stats()
    return 1e3 * dt / iters, st.matvec_ms / max(st.matvec_count, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("poisson", "banded"), required=True)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--logn", type=int, default=20)
    ap.add_argument("--hb", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose conjugate_gradient_amd is loaded")
    ap.add_argument("--solve", type=float, default=None, metavar="DEC")
    ap.add_argument("--plain-cap", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import conjugate_gradient_amd as cg
    ab = load(os.path.join(HERE, "spmv_ab.py"), "spmv_ab")
    out = args.out or os.path.join("profiles", f"pcg_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    if args.matrix == "poisson":
        indptr, indices, data = ab.poisson_csr(args.m)
        label = f"poisson m={args.m}"
    else:
        indptr, indices, data = ab.banded_csr(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    n, nnz = indptr.size - 1, int(indptr[-1])
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    forms = ("plain",) if args.plain_only else ("plain", "jacobi")

    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        s = cg.Solver.from_csr(indptr, indices, data, flags=cg.CGX_F64 | cg.CGX_TIMING)
        plan = s.matvec_plan()
        extract_ms = []
        if not args.plain_only:
            for _ in range(4):  # the first call loads the code object and allocates: reported apart
                t0 = time.perf_counter()
                s.set_precond("jacobi")
                extract_ms.append(1e3 * (time.perf_counter() - t0))

        def setup(form):
            if not args.plain_only:
                s.set_precond("jacobi" if form == "jacobi" else None)

        emit({"record": "setup", "matrix": label, "n": n, "nnz": nnz, "library": os.path.relpath(args.root),
              "plan": plan, "rounds": args.rounds, "iters": args.iters, "forms": forms,
              "extract_first_ms": extract_ms[0] if extract_ms else None,
              "extract_ms": statistics.median(extract_ms[1:]) if extract_ms else None})
        t_end = time.perf_counter() + args.settle
        while time.perf_counter() < t_end:
            for form in forms:
                setup(form)
                time_form(s, 5)
        it = {form: [] for form in forms}
        mv = {form: [] for form in forms}
        for r in range(args.rounds):
            for form in (forms if r % 2 == 0 else forms[::-1]):
                setup(form)
                a, b = time_form(s, args.iters)
                it[form].append(a)
                mv[form].append(b)
                emit({"record": "round", "round": r, "form": form, "iteration_ms": a, "spmv_ms": b,
                      "updates_ms": a - b})

        def summ(form):
            upd = [a - b for a, b in zip(it[form], mv[form])]
            med = statistics.median(it[form])
            return {"iteration_ms": med, "iteration_spread": (max(it[form]) - min(it[form])) / med,
                    "spmv_ms": statistics.median(mv[form]), "updates_ms": statistics.median(upd),
                    "updates_tbs": (PCG_B if form == "jacobi" else PLAIN_B) * n / (statistics.median(upd) * 1e-3) / 1e12}

        summary = {"record": "summary", "matrix": label, **{form: summ(form) for form in forms}}
        if not args.plain_only:
            p, j = summary["plain"], summary["jacobi"]
            summary["jacobi_over_plain"] = j["iteration_ms"] / p["iteration_ms"]
            # +16 B per row on top of the plain iteration's time, at the rate the plain update kernels reach
            summary["expected_jacobi_ms"] = p["iteration_ms"] + 16.0 * n / (PLAIN_B * n / p["updates_ms"])
        emit(summary)

        if args.solve is not None and not args.plain_only:
            h = np.sqrt(10.0 ** (args.solve * ((np.arange(n, dtype=np.int64) * 7919) % n) / n))
            rows = np.repeat(np.arange(n), np.diff(indptr))
            s.set_csr(indptr, indices, data * h[rows] * h[indices])
            b = h * np.ones(n)
            eps = 1e-8 * float(np.linalg.norm(b))
            rec = {"record": "solve", "matrix": label, "decades": args.solve, "eps": eps, "plain_cap": args.plain_cap}
            for form, cap in (("jacobi", -1), ("plain", args.plain_cap)):  # -1: n loops, the library's own cap
                s.set_precond("jacobi" if form == "jacobi" else None)
                s.set_rows(0, b_rows=b, x_rows=np.zeros(n))
                s.synchronize()
                t0 = time.perf_counter()
                _, st = s.solve(eps=eps, max_iter=cap)
                wall = time.perf_counter() - t0
                rn, bn = s.residual_norm()
                rec[form] = {"loops": st.iterations, "converged": st.converged, "wall_ms": 1e3 * wall,
                             "solve_ms": st.solve_ms, "true_residual_over_b": rn / bn,
                             "cap_hit": bool(st.converged == 0 and st.iterations >= (cap if cap >= 0 else n))}
            emit(rec)
        s.close()


if __name__ == "__main__":
    main()
