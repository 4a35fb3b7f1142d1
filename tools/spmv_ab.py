#!/usr/bin/env python3
"""Sweep every instantiated plan (T lanes per row, load policy) of the CSR SpMV kernel (k_csr_mult_f64 at K = 1) on one
GPU, against the vendor library's CSR product reached through torch (torch.sparse_csr_tensor(...) @ v), in
interleaved rounds in one process.

Two matrices, built with numpy from nothing but their sizes:
  poisson  the 5-point matrix of an m x m grid (default m = 4096: 16.8 M rows, 83.9 M entries, mean row length 5)
  banded   n = 2^20 rows, half-bandwidth 32 (65 entries per full row): off-diagonals from a counter hash
           (symmetric), diagonal = row sum of absolute values + 1 (so SPD)

Protocol: a settle, then --rounds interleaved rounds; in each round every (T, policy), the context's default plan
and the torch product run once, --iters launches each after one warm launch.  The matVec is timed by the
context's CGX_TIMING events (torch: torch.cuda events around the same number of products); the iteration by
fixed-count iterations bracketed by synchronize.  One JSON line per round and configuration, then one summary
line with the medians, the round-to-round spread and the default plan's ratio to torch.  GB/s are on the
algorithmic bytes 12 nnz + 8 (n + 1) + 16 n (8 nnz with --a-f32).  For poisson the matrix-free
Solver(poisson_m=m) iteration rate is recorded too (context, not a target: it moves 58.7 B per point).

  python tools/spmv_ab.py --matrix poisson [--m 4096] [--rounds 5] [--iters 20] [--out profiles/spmv_ab_poisson.jsonl]
  python tools/spmv_ab.py --matrix banded [--logn 20] [--hb 32]
  --a-f32: float-stored values (cgx_set_csr_f32; the values are rounded to float first, for torch too)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import conjugate_gradient_amd as cg  # noqa: E402

TS = (2, 4, 8, 16, 32, 64)
POLICIES = (2, 8)


def poisson_csr(m):
    n = m * m
    k = np.arange(n, dtype=np.int32)
    i, j = k // m, k % m
    cand = np.stack([k - m, k - 1, k, k + 1, k + m], axis=1)
    valid = np.stack([i > 0, j > 0, np.ones(n, bool), j < m - 1, i < m - 1], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (n, 5))
    indptr = np.concatenate([[0], np.cumsum(valid.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    return indptr, np.ascontiguousarray(cand[valid]), np.ascontiguousarray(vals[valid])


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def banded_csr(n, hb):
    i = np.arange(n, dtype=np.int64)[:, None]
    cand = i + np.arange(-hb, hb + 1, dtype=np.int64)[None, :]
    valid = (cand >= 0) & (cand < n)
    lo, hi = np.minimum(i, cand).astype(np.uint64), np.maximum(i, cand).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _mix64((lo << np.uint64(32)) | hi)
    vals = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5  # symmetric: a function of (min, max)
    vals[~valid] = 0.0
    vals[:, hb] = 0.0
    vals[:, hb] = np.abs(vals).sum(axis=1) + 1.0
    indptr = np.concatenate([[0], np.cumsum(valid.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    return indptr, np.ascontiguousarray(cand[valid].astype(np.int32)), np.ascontiguousarray(vals[valid])


def time_plan(s, plan, iters):
    """(ms per matVec launch by CGX_TIMING events, ms per iteration by the host clock around a synchronize) of
    `iters` fixed-count iterations under `plan` = (T, policy), or the plan the context has (None)."""
    if plan is not None:
        s.set_matvec_plan(64 // plan[0], 1, plan[1])
    s.fill(1.0, 0.0)
    s.begin()
    s.iterate(1, eps=-1.0)  # warm this plan
    s.reset_timing()
    s.synchronize()
    t0 = time.perf_counter()
    s.iterate(iters, eps=-1.0)
    s.synchronize()
    dt = time.perf_counter() - t0
    st = s.stats()
    assert st.matvec_count == iters
    return st.matvec_ms / st.matvec_count, 1e3 * dt / iters


def torch_setup(indptr, indices, data, n):
    """(product closure, description) or (None, why not)."""
    try:
        import torch
        if not torch.cuda.is_available():
            return None, "torch sees no GPU"
        dev = torch.device("cuda:0")
        v = torch.ones(n, dtype=torch.float64, device=dev)
        last = None
        for idt in (torch.int32, torch.int64):
            if idt == torch.int32 and indptr[-1] >= 2 ** 31:
                continue
            try:
                A = torch.sparse_csr_tensor(torch.from_numpy(indptr).to(dev, idt), torch.from_numpy(indices).to(dev, idt),
                                            torch.from_numpy(data).to(dev), size=(n, n))
                y = A @ v
                torch.cuda.synchronize()
                return (torch, A, v, y), f"torch {torch.__version__}, {str(idt).split('.')[-1]} indices"
            except Exception as e:  # noqa: BLE001
                last = e
        return None, f"torch CSR product failed: {last!r}"
    except Exception as e:  # noqa: BLE001
        return None, f"torch unavailable: {e!r}"


def time_torch(tc, iters):
    torch, A, v, _ = tc
    A @ v  # warm
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        A @ v
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=("poisson", "banded"), required=True)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--logn", type=int, default=20)
    ap.add_argument("--hb", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--a-f32", action="store_true", help="float-stored values (cgx_set_csr_f32)")
    ap.add_argument("--torch-first", action="store_true",
                    help="initialise torch's GPU runtime before libcgx is loaded (a torch wheel that bundles its own "
                         "HIP runtime finds no GPU once another copy of the runtime has opened the device)")
    args = ap.parse_args()
    out = args.out or os.path.join("profiles", f"spmv_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    t0 = time.perf_counter()
    if args.matrix == "poisson":
        indptr, indices, data = poisson_csr(args.m)
        label = f"poisson m={args.m}"
    else:
        indptr, indices, data = banded_csr(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    if args.a_f32:
        data = data.astype(np.float32).astype(np.float64)
    n, nnz = indptr.size - 1, int(indptr[-1])
    abytes = (8 if args.a_f32 else 12) * nnz + 8 * (n + 1) + 16 * n
    build_s = time.perf_counter() - t0

    def gbs(ms):
        return abytes / (ms * 1e-3) / 1e9

    if args.torch_first:
        import torch
        if torch.cuda.is_available():
            torch.zeros(1, device="cuda:0")
            torch.cuda.synchronize()
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    s = cg.Solver.from_csr(indptr, indices, data, flags=cg.CGX_F64 | cg.CGX_TIMING, a_f32=args.a_f32)
    default = s.matvec_plan()
    default_plan = (64 // default["R"], default["nt"])
    tc, torch_note = torch_setup(indptr, indices, data, n)
    check = None
    if tc is not None:  # the same product at the timed size: the kernel against the vendor library
        dv, do = cg.DeviceArray.from_host(np.ones(n)), cg.DeviceArray(n)
        os.environ["CGX_SPMV_PLAN"] = f"T={default_plan[0]},nt={default_plan[1]}"
        cg.spmv_csr(indptr, indices, data, dv, do, n, n, a_f32=args.a_f32)
        del os.environ["CGX_SPMV_PLAN"]
        mine, theirs = do.to_host(), tc[3].cpu().numpy()
        check = float(np.max(np.abs(mine - theirs)) / max(np.max(np.abs(theirs)), 1e-300))
        dv.free()
        do.free()
    pois = cg.Solver(None, poisson_m=args.m) if args.matrix == "poisson" else None

    configs = [(T, nt) for T in TS for nt in POLICIES]
    t_end = time.perf_counter() + args.settle  # settle: clocks up, code objects loaded, every plan launched once
    while time.perf_counter() < t_end:
        for c in configs:
            time_plan(s, c, 2)
        if tc is not None:
            time_torch(tc, 2)
    ms = {c: [] for c in configs}
    ms["default"], ms["torch"], it_ms, pois_its = [], [], [], []
    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        emit({"record": "setup", "matrix": label, "values": "float" if args.a_f32 else "double", "n": n, "nnz": nnz,
              "algorithmic_bytes": abytes,
              "build_s": round(build_s, 2), "default_plan": {"T": default_plan[0], "nt": default_plan[1],
                                                             "blocks": default["blocks"]},
              "torch": torch_note, "max_rel_diff_vs_torch": check, "rounds": args.rounds, "iters": args.iters})
        for r in range(args.rounds):
            order = configs if r % 2 == 0 else configs[::-1]
            for c in order:
                m, _ = time_plan(s, c, args.iters)
                ms[c].append(m)
                emit({"record": "round", "round": r, "config": f"T={c[0]},nt={c[1]}", "ms": m, "gbs": gbs(m)})
            s.set_matvec_plan(64 // default_plan[0], 1, default_plan[1])
            m, it = time_plan(s, None, args.iters)
            ms["default"].append(m)
            it_ms.append(it)
            emit({"record": "round", "round": r, "config": "default", "ms": m, "gbs": gbs(m), "iteration_ms": it,
                  "iterations_per_s": 1e3 / it})
            if tc is not None:
                m = time_torch(tc, args.iters)
                ms["torch"].append(m)
                emit({"record": "round", "round": r, "config": "torch_csr_matvec", "ms": m, "gbs": gbs(m)})
            if pois is not None:
                pois.fill(1.0, 0.0)
                pois.begin()
                pois.iterate(3, eps=-1.0)
                pois.synchronize()
                t1 = time.perf_counter()
                pois.iterate(args.iters, eps=-1.0)
                pois.synchronize()
                rate = args.iters / (time.perf_counter() - t1)
                pois_its.append(rate)
                emit({"record": "round", "round": r, "config": "matrix_free_poisson", "iterations_per_s": rate})

        def summ(v):
            return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                    "median_gbs": gbs(statistics.median(v))} if v else None

        summary = {"record": "summary", "matrix": label,
                   "plans": {f"T={c[0]},nt={c[1]}": summ(ms[c]) for c in configs},
                   "default": summ(ms["default"]), "torch_csr_matvec": summ(ms["torch"]),
                   "default_iteration_ms_median": statistics.median(it_ms)}
        if ms["torch"]:
            summary["default_over_torch"] = statistics.median(ms["default"]) / statistics.median(ms["torch"])
        if pois_its:
            summary["matrix_free_poisson_iterations_per_s_median"] = statistics.median(pois_its)
        best = min(configs, key=lambda c: statistics.median(ms[c]))
        summary["best_plan"] = f"T={best[0]},nt={best[1]}"
        emit(summary)
    s.close()


if __name__ == "__main__":
    main()
