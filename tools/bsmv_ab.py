#!/usr/bin/env python3
"""The block SpMV (k_bsr_mult_f64, csrc/cgx_bsmv.hip) against the CSR SpMV (k_csr_mult_f64) on the expanded matrix,
and its tiled device layout against the plain one, on one GPU, in interleaved rounds in one process.

Three families, every (T lanes per [block] row, load policy) of each:
  tiled  the library's kernel (cgx_bsr_tile_values once, then cgx_spmv_bsr under CGX_BSMV_PLAN)
  plain  the same kernel reading scipy's layout as it stands (tools/microbench/bsmv_plain.hip, built by this tool;
         bs = 3 and 4 only)
  csr    cgx_spmv_csr under CGX_SPMV_PLAN on the expanded matrix (every block's bs^2 entries, zeros included:
         the blocks of these matrices are full)
All three are kernel-level launches on the null stream, timed alike by one pair of events around --iters launches
after one warm launch (bsmv_timer_start / bsmv_timer_stop of the microbenchmark library).

Two matrices, built with numpy from nothing but their sizes, each with at least 0.5 GB of values so that the 256 MiB
Infinity Cache does not hold them:
  grid    the block 5-point matrix of an m x m grid of nodes (default m = 1200: 1.44 M block rows, 7.2 M blocks;
          0.52 GB of values at bs = 3, 0.92 GB at bs = 4)
  banded  nb = 2^18 block rows, 27 blocks per full block row (half-bandwidth 13), bs = 3 (0.51 GB)
The diagonal blocks are (4 + bs) I + a small symmetric part (positive definite, so block Jacobi sets up); the matrix
as a whole is not made symmetric -- nothing here is solved.

--iteration: also the time of a fixed-count CG iteration of a block-valued context and of a CSR context on the
expanded matrix, plain and with block Jacobi at pbs = bs, each at its default plan, in the same rounds.

One JSON line per round and configuration, then a summary with the medians, the best plan of each family and the
ratios csr / tiled and plain / tiled beside the byte model's 12 / (8 + 4 / bs^2).  GB/s are on the algorithmic bytes:
nnzb (8 bs^2 + 4) + 8 (nb + 1) + 16 n for BSR, 12 nnz + 8 (n + 1) + 16 n for CSR.

  python tools/bsmv_ab.py --matrix grid --bs 3 [--m 1200] [--rounds 5] [--iters 10] [--iteration] [--out FILE]
  python tools/bsmv_ab.py --matrix banded --bs 3 [--lognb 18] [--hb 13]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import conjugate_gradient_amd as cg  # noqa: E402

TS = (2, 4, 8, 16, 32, 64)
POLICIES = (2, 8)
MB_DIR = os.path.join(ROOT, "tools", "microbench")
MB_LIB = os.path.join(MB_DIR, "libbsmv_plain.so")


def microbench_lib():
    src = os.path.join(MB_DIR, "bsmv_plain.hip")
    if not os.path.exists(MB_LIB) or os.path.getmtime(MB_LIB) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-shared", "-fPIC", "-o", MB_LIB, src], check=True)
    L = ctypes.CDLL(MB_LIB)
    vp = ctypes.c_void_p
    L.bsmv_plain_launch.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, vp, vp, vp, vp, vp]
    L.bsmv_plain_launch.restype = ctypes.c_int
    L.bsmv_timer_start.restype = ctypes.c_int
    L.bsmv_timer_stop.restype = ctypes.c_float
    return L


def structure(cand, valid):
    indptr = np.concatenate([[0], np.cumsum(valid.sum(axis=1, dtype=np.int64))]).astype(np.int64)
    return indptr, np.ascontiguousarray(cand[valid].astype(np.int32))


def grid_structure(m):
    nb = m * m
    k = np.arange(nb, dtype=np.int64)
    i, j = k // m, k % m
    cand = np.stack([k - m, k - 1, k, k + 1, k + m], axis=1)
    valid = np.stack([i > 0, j > 0, np.ones(nb, bool), j < m - 1, i < m - 1], axis=1)
    return structure(cand, valid)


def banded_structure(nb, hb):
    cand = np.arange(nb, dtype=np.int64)[:, None] + np.arange(-hb, hb + 1, dtype=np.int64)[None, :]
    return structure(cand, (cand >= 0) & (cand < nb))


def block_values(indptr, indices, bs, seed=1):
    """(nnzb, bs, bs): off-diagonal blocks -I / 4 + noise, diagonal blocks (4 + bs) I + a small symmetric part."""
    rng = np.random.default_rng(seed)
    nb = indptr.size - 1
    data = 0.05 * rng.standard_normal((indices.size, bs, bs))
    data -= 0.25 * np.eye(bs)
    diag = np.flatnonzero(indices == np.repeat(np.arange(nb), np.diff(indptr)))
    d = data[diag]
    data[diag] = 0.5 * (d + d.transpose(0, 2, 1)) + (4.25 + bs) * np.eye(bs)
    return data


def expand(indptr, indices, data):
    """The scalar CSR arrays: row I bs + i lists its blocks' entries block after block, j ascending."""
    nb, bs = indptr.size - 1, data.shape[1]
    seg_len = np.repeat(np.diff(indptr), bs)
    seg_start = np.repeat(indptr[:-1], bs)
    ends = np.cumsum(seg_len)
    q_of = np.repeat(seg_start - (ends - seg_len), seg_len) + np.arange(int(ends[-1]), dtype=np.int64)
    i_of = np.repeat(np.tile(np.arange(bs), nb), seg_len)
    rp = np.concatenate([[0], ends * bs]).astype(np.int64)
    ci = (indices[q_of].astype(np.int64)[:, None] * bs + np.arange(bs)[None, :]).reshape(-1).astype(np.int32)
    va = np.ascontiguousarray(data[q_of, i_of, :]).reshape(-1)
    return rp, ci, va


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
    ap.add_argument("--matrix", choices=("grid", "banded"), required=True)
    ap.add_argument("--bs", type=int, required=True)
    ap.add_argument("--m", type=int, default=1200)
    ap.add_argument("--lognb", type=int, default=18)
    ap.add_argument("--hb", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--iteration", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bs = args.bs
    out = args.out or os.path.join("profiles", f"bsmv_ab_{args.matrix}_bs{bs}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)

    t0 = time.perf_counter()
    if args.matrix == "grid":
        indptr, indices = grid_structure(args.m)
        label = f"block 5-point grid m={args.m} bs={bs}"
    else:
        indptr, indices = banded_structure(1 << args.lognb, args.hb)
        label = f"block banded nb=2^{args.lognb} hb={args.hb} bs={bs}"
    data = block_values(indptr, indices, bs)
    rp, ci, va = expand(indptr, indices, data)
    nb, nnzb = indptr.size - 1, int(indices.size)
    n, nnz = nb * bs, int(ci.size)
    bsr_bytes = nnzb * (8 * bs * bs + 4) + 8 * (nb + 1) + 16 * n
    csr_bytes = 12 * nnz + 8 * (n + 1) + 16 * n
    build_s = time.perf_counter() - t0
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")
    MB, L = microbench_lib(), cg.lib()
    plain_ok = bs in (3, 4)

    DA = cg.DeviceArray
    d_brp, d_bci, d_val = DA.from_host(indptr), DA.from_host(indices), DA.from_host(data.reshape(-1))
    d_tiled = DA((nnzb + 63) // 64 * 64 * bs * bs)
    d_rp, d_ci, d_va = DA.from_host(rp), DA.from_host(ci), DA.from_host(va)
    v = np.random.default_rng(2).standard_normal(n)
    d_v, d_out = DA.from_host(v), DA(n)
    assert L.cgx_bsr_tile_values(nnzb, bs, d_val.ptr, d_tiled.ptr, None) == 0, L.cgx_last_error()

    def launch(family, T, nt):
        if family == "tiled":
            os.environ["CGX_BSMV_PLAN"] = f"T={T},nt={nt}"
            rc = L.cgx_spmv_bsr(nb, nb, bs, d_brp.ptr, d_bci.ptr, d_tiled.ptr, d_v.ptr, d_out.ptr, None)
        elif family == "plain":
            rc = MB.bsmv_plain_launch(bs, T, nt, nb, d_brp.ptr, d_bci.ptr, d_val.ptr, d_v.ptr, d_out.ptr)
        else:
            os.environ["CGX_SPMV_PLAN"] = f"T={T},nt={nt}"
            rc = L.cgx_spmv_csr(n, n, d_rp.ptr, d_ci.ptr, d_va.ptr, d_v.ptr, d_out.ptr, None)
        assert rc == 0, (family, T, nt, rc, L.cgx_last_error())

    def timed(family, T, nt, iters):
        launch(family, T, nt)  # warm
        assert MB.bsmv_timer_start() == 0
        for _ in range(iters):
            launch(family, T, nt)
        ms = MB.bsmv_timer_stop()
        assert ms > 0
        return ms / iters

    families = ("tiled",) + (("plain",) if plain_ok else ()) + ("csr",)
    # the three families compute the same product (different orders): checked once at the timed size
    outs = {}
    for fam in families:
        launch(fam, 8, 2)
        assert L.cgx_dev_synchronize() == 0
        outs[fam] = d_out.to_host()
    scale = float(np.max(np.abs(outs["csr"])))
    check = {fam: float(np.max(np.abs(outs[fam] - outs["csr"])) / scale) for fam in families}
    assert all(c <= 1e-12 for c in check.values()), check

    ctxs = {}
    if args.iteration:
        for name in ("CGX_BSMV_PLAN", "CGX_SPMV_PLAN"):  # the contexts run their default plans
            os.environ.pop(name, None)
        for name, make in (("bsr", lambda p: cg.Solver.from_bsr(indptr, indices, data, precond=p)),
                           ("csr", lambda p: cg.Solver.from_csr(rp, ci, va, precond=p))):
            for pname, p in (("plain", None), ("block_jacobi", ("block", bs))):
                ctxs[f"{name}_{pname}"] = make(p)

    configs = [(fam, T, nt) for fam in families for T in TS for nt in POLICIES]
    t_end = time.perf_counter() + args.settle  # settle: clocks up, code objects loaded, every plan launched once
    while time.perf_counter() < t_end:
        for c in configs:
            timed(*c, 1)
    ms = {c: [] for c in configs}
    it_ms = {k: [] for k in ctxs}
    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        emit({"record": "setup", "matrix": label, "nb": nb, "nnzb": nnzb, "n": n, "nnz": nnz,
              "values_gb": nnzb * bs * bs * 8 / 1e9, "bsr_bytes": bsr_bytes, "csr_bytes": csr_bytes,
              "byte_model_ratio": 12.0 / (8.0 + 4.0 / (bs * bs)), "build_s": round(build_s, 2),
              "max_rel_diff_vs_csr": check, "rounds": args.rounds, "iters": args.iters,
              "default_plans": {k: s.matvec_plan() for k, s in ctxs.items()}})
        for r in range(args.rounds):
            for c in (configs if r % 2 == 0 else configs[::-1]):
                m = timed(*c, args.iters)
                ms[c].append(m)
                emit({"record": "round", "round": r, "family": c[0], "T": c[1], "nt": c[2], "ms": m,
                      "gbs": (csr_bytes if c[0] == "csr" else bsr_bytes) / (m * 1e-3) / 1e9})
            for k, s in ctxs.items():
                m = time_iteration(s, 5 * args.iters)
                it_ms[k].append(m)
                emit({"record": "round", "round": r, "context": k, "iteration_ms": m})

        med = {c: statistics.median(v) for c, v in ms.items()}
        best = {fam: min((c for c in configs if c[0] == fam), key=med.get) for fam in families}
        summary = {"record": "summary", "matrix": label,
                   "median_ms": {fam: {f"T={T},nt={nt}": med[fam, T, nt] for T in TS for nt in POLICIES}
                                 for fam in families},
                   "spread": {fam: max((max(ms[c]) - min(ms[c])) / med[c] for c in configs if c[0] == fam)
                              for fam in families},
                   "best": {fam: {"T": best[fam][1], "nt": best[fam][2], "ms": med[best[fam]],
                                  "gbs": (csr_bytes if fam == "csr" else bsr_bytes) / (med[best[fam]] * 1e-3) / 1e9}
                            for fam in families},
                   "csr_over_tiled": med[best["csr"]] / med[best["tiled"]],
                   "byte_model_ratio": 12.0 / (8.0 + 4.0 / (bs * bs))}
        if plain_ok:
            summary["plain_over_tiled"] = med[best["plain"]] / med[best["tiled"]]
        if ctxs:
            summary["iteration_ms_median"] = {k: statistics.median(v) for k, v in it_ms.items()}
        emit(summary)
    for s in ctxs.values():
        s.close()


if __name__ == "__main__":
    main()
