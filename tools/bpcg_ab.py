#!/usr/bin/env python3
"""Block-Jacobi preconditioned CG against the plain and the Jacobi iteration on a cgx_create_csr context, one GPU,
in interleaved rounds in one process -- what the block update kernels (cgx_pcg_block.hip) cost per iteration beside
their byte model.

The matrix is tools/spmv_ab.py's 5-point Poisson matrix of an m x m grid (default m = 4096, 16.8 M rows: each vector
is 134 MB, beyond the caches).  Its diagonal blocks are positive definite for every block size.

Protocol (tools/pcg_ab.py's): a settle, then --rounds interleaved rounds; in each round every form runs --iters
fixed-count iterations after a warm one, the order reversed every other round.  Per form and round: ms per iteration
by the host clock around a synchronize, ms per SpMV launch by the context's CGX_TIMING events, and their difference
-- the two update kernels with the launch gaps, which is where the forms differ.  Bytes per row of the two update
kernels: plain 24 + 40, Jacobi 32 + 48, block (32 + 8 bs) + 40.  One JSON line per round and form, then a summary
with the medians, the spread ((max - min) / median), the update kernels' TB/s on those bytes, what the byte model
predicts for each block form from the Jacobi form measured in the same run, and the one-time set-up
(cgx_set_precond_block: extract, download, invert on the host, upload).

  python tools/bpcg_ab.py [--m 4096] [--bs 2,4,8] [--rounds 5] [--iters 50] [--out profiles/bpcg_ab_poisson.jsonl]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def update_bytes(form):
    if form == "plain":
        return 24 + 40
    if form == "jacobi":
        return 32 + 48
    return 32 + 8 * int(form[5:]) + 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--bs", default="2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import conjugate_gradient_amd as cg
    ab = load(os.path.join(HERE, "spmv_ab.py"), "spmv_ab")
    time_form = load(os.path.join(HERE, "pcg_ab.py"), "pcg_ab").time_form
    out = args.out or os.path.join("profiles", "bpcg_ab_poisson.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    indptr, indices, data = ab.poisson_csr(args.m)
    n, nnz = indptr.size - 1, int(indptr[-1])
    sizes = [int(v) for v in args.bs.split(",")]
    forms = ("plain", "jacobi", *(f"block{b}" for b in sizes))

    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        s = cg.Solver.from_csr(indptr, indices, data, flags=cg.CGX_F64 | cg.CGX_TIMING)
        setup_ms = {}

        def setup(form):
            t0 = time.perf_counter()
            if form == "plain":
                s.set_precond(None)
            elif form == "jacobi":
                s.set_precond("jacobi")
            else:
                s.set_precond_block(int(form[5:]))
            setup_ms.setdefault(form, []).append(1e3 * (time.perf_counter() - t0))

        emit({"record": "setup", "matrix": f"poisson m={args.m}", "n": n, "nnz": nnz, "plan": s.matvec_plan(),
              "rounds": args.rounds, "iters": args.iters, "forms": forms})
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
                    "update_bytes_per_row": update_bytes(form),
                    "updates_tbs": update_bytes(form) * n / (statistics.median(upd) * 1e-3) / 1e12,
                    "setup_first_ms": setup_ms[form][0], "setup_ms": statistics.median(setup_ms[form][1:])}

        summary = {"record": "summary", "matrix": f"poisson m={args.m}", **{form: summ(form) for form in forms}}
        j = summary["jacobi"]
        for form in forms[2:]:  # the byte model: the Jacobi update kernels' measured rate on the block form's bytes
            b = summary[form]
            b["model_updates_ms"] = j["updates_ms"] * update_bytes(form) / update_bytes("jacobi")
            b["updates_over_model"] = b["updates_ms"] / b["model_updates_ms"]
        emit(summary)
        s.close()


if __name__ == "__main__":
    main()
