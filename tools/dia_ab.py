#!/usr/bin/env python3
"""The diagonal-storage SpMV (k_dia_mult_f64, csrc/cgx_dia.hip) against the CSR SpMV (k_csr_mult_f64) on the same
matrix, on one GPU, in interleaved rounds in one process.

Two families:
  dia  cgx_spmv_dia under CGX_DIA_PLAN, every (R rows per lane, U diagonals in flight, load policy)
  csr  cgx_spmv_csr under CGX_SPMV_PLAN, every (T lanes per row, load policy): its best plan is the comparison
Both are kernel-level launches on the null stream, timed alike by one pair of HIP events around --iters launches after
one warm launch.

The two matrices every sparse measurement of the project uses, built with numpy from nothing but their sizes:
  poisson  the 5-point matrix of an m x m grid (default m = 4096: 16.8 M rows, 5 diagonals; the +-1 diagonals hold a
           stored zero where a grid row ends, which the CSR arrays do not list)
  banded   n = 2^20 rows, 65 entries per full row (half-bandwidth 32), 65 diagonals

--iteration: also the time of a fixed-count CG iteration of a diagonal-valued context and of a CSR context, plain and
with Jacobi, each at its default plan, in the same rounds.

One JSON line per round and configuration, then a summary with the medians, the best plan of each family and the
ratio csr / dia beside the byte model's.  GB/s are on the algorithmic bytes: 8 ndiag n + 16 n for DIA,
12 nnz + 8 (n + 1) + 16 n for CSR.

  python tools/dia_ab.py --matrix poisson [--m 4096] [--rounds 5] [--iters 10] [--iteration] [--out FILE]
  python tools/dia_ab.py --matrix banded [--logn 20] [--hb 32]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import conjugate_gradient_amd as cg  # noqa: E402

RS, US, POLICIES = (1, 2), (1, 2, 4, 8), (2, 8)
TS = (2, 4, 8, 16, 32, 64)


class Events:
    """One pair of HIP events on the null stream."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.e[0], None) == 0

    def stop(self):
        assert self.hip.hipEventRecord(self.e[1], None) == 0
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.e[0], self.e[1]) == 0
        return ms.value


def poisson_dia(m):
    n = m * m
    j = np.arange(n, dtype=np.int64)
    offsets = np.array([-m, -1, 0, 1, m], np.int32)
    data = np.empty((5, n))
    data[0], data[4], data[2] = -1.0, -1.0, 4.0
    data[1] = np.where((j + 1) % m != 0, -1.0, 0.0)  # A[j + 1][j]
    data[3] = np.where(j % m != 0, -1.0, 0.0)  # A[j - 1][j]
    return offsets, data


def banded_dia(n, hb, seed=1):
    """Symmetric, diagonally dominant: A[i][i + d] = A[i + d][i] in [-0.5, 0.5) / hb, the diagonal in [4, 5)."""
    rng = np.random.default_rng(seed)
    offsets = np.arange(-hb, hb + 1, dtype=np.int32)
    data = np.zeros((2 * hb + 1, n))
    data[hb] = 4.0 + rng.random(n)
    for d in range(1, hb + 1):
        c = (rng.random(n - d) - 0.5) / hb  # c[i] = A[i][i + d]
        data[hb + d, d:] = c  # slot = the column i + d
        data[hb - d, :n - d] = c  # A[i + d][i]: slot = the column i
    return offsets, data


def to_csr(offsets, data, n):
    """The CSR arrays of the matrix: columns ascending (the offsets are), in-range entries, zeros not listed."""
    rows = np.arange(n, dtype=np.int64)
    cols = np.empty((n, offsets.size), np.int64)
    vals = np.empty((n, offsets.size))
    keep = np.empty((n, offsets.size), bool)
    for k, o in enumerate(offsets.astype(np.int64)):
        c = rows + o
        ok = (c >= 0) & (c < n)
        cc = np.clip(c, 0, n - 1)
        cols[:, k], vals[:, k] = c, data[k, cc]
        keep[:, k] = ok & (vals[:, k] != 0.0)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    return rp, cols[keep].astype(np.int32), np.ascontiguousarray(vals[keep])


def time_iteration(s, iters):
    """ms per fixed-count iteration by the host clock around a synchronize."""
    s.fill(1.0, 0.0)
    s.begin()
    s.iterate(2, eps=-1.0)
    s.synchronize()
    t0 = time.perf_counter()
    s.iterate(iters, eps=-1.0)
    s.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


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
    out = args.out or os.path.join("profiles", f"dia_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    t0 = time.perf_counter()
    if args.matrix == "poisson":
        offsets, data = poisson_dia(args.m)
        label = f"5-point Poisson m={args.m}"
    else:
        offsets, data = banded_dia(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    n, ndiag = data.shape[1], int(offsets.size)
    rp, ci, va = to_csr(offsets, data, n)
    nnz = int(ci.size)
    dia_bytes = 8 * ndiag * n + 16 * n
    csr_bytes = 12 * nnz + 8 * (n + 1) + 16 * n
    build_s = time.perf_counter() - t0
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    L, ev = cg.lib(), Events()

    DA = cg.DeviceArray
    d_off, d_data = DA.from_host(offsets), DA.from_host(data.reshape(-1))
    d_rp, d_ci, d_va = DA.from_host(rp), DA.from_host(ci), DA.from_host(va)
    v = np.random.default_rng(2).standard_normal(n)
    d_v, d_out = DA.from_host(v), DA(n)

    def launch(family, a, b, nt):
        if family == "dia":
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

    # the two families compute the same product (different orders): checked once at the timed size
    outs = {}
    for fam, c in (("dia", ("dia", 2, 4, 2)), ("csr", ("csr", 8, 0, 2))):
        launch(*c)
        assert L.cgx_dev_synchronize() == 0
        outs[fam] = d_out.to_host()
    check = float(np.max(np.abs(outs["dia"] - outs["csr"])) / np.max(np.abs(outs["csr"])))
    assert check <= 1e-12, check

    ctxs = {}
    if args.iteration:
        for name in ("CGX_DIA_PLAN", "CGX_SPMV_PLAN"):  # the contexts run their default plans
            os.environ.pop(name, None)
        for name, make in (("dia", lambda p: cg.Solver.from_dia(offsets, data, precond=p)),
                           ("csr", lambda p: cg.Solver.from_csr(rp, ci, va, precond=p))):
            for pname, p in (("plain", None), ("jacobi", "jacobi")):
                ctxs[f"{name}_{pname}"] = make(p)

    configs = [("dia", R, U, nt) for R in RS for U in US for nt in POLICIES] + \
              [("csr", T, 0, nt) for T in TS for nt in POLICIES]
    key = lambda c: f"R={c[1]},U={c[2]},nt={c[3]}" if c[0] == "dia" else f"T={c[1]},nt={c[3]}"  # noqa: E731
    nbytes = {"dia": dia_bytes, "csr": csr_bytes}
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

        model = csr_bytes / dia_bytes
        emit({"record": "setup", "matrix": label, "n": n, "ndiag": ndiag, "nnz": nnz, "dia_values_gb": ndiag * n * 8 / 1e9,
              "dia_bytes": dia_bytes, "csr_bytes": csr_bytes, "byte_model_ratio": model, "build_s": round(build_s, 2),
              "max_rel_diff_vs_csr": check, "rounds": args.rounds, "iters": args.iters,
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
        best = {fam: min((c for c in configs if c[0] == fam), key=med.get) for fam in ("dia", "csr")}
        summary = {"record": "summary", "matrix": label,
                   "median_ms": {fam: {key(c): med[c] for c in configs if c[0] == fam} for fam in ("dia", "csr")},
                   "spread": {fam: max((max(ms[c]) - min(ms[c])) / med[c] for c in configs if c[0] == fam)
                              for fam in ("dia", "csr")},
                   "best": {fam: {"plan": key(best[fam]), "ms": med[best[fam]],
                                  "gbs": nbytes[fam] / (med[best[fam]] * 1e-3) / 1e9} for fam in ("dia", "csr")},
                   "csr_over_dia": med[best["csr"]] / med[best["dia"]], "byte_model_ratio": model}
        if ctxs:
            summary["iteration_ms_median"] = {k: statistics.median(t) for k, t in it_ms.items()}
        emit(summary)
    for s in ctxs.values():
        s.close()


if __name__ == "__main__":
    main()
