#!/usr/bin/env python3
"""A sparse A over row blocks (cgx_create_csr_multi) against one block (cgx_create_csr), and its indexed exchange
(CGX_CSR_XCHG=index, k_gather_indexed) against the whole-slice one (CGX_CSR_XCHG=full, k_gather_slices), every block
on device 0.  One device can only repeat itself: this measures the kernels and the host's enqueue, not a link, and
says nothing about scaling over GPUs.

The two matrices are tools/spmv_ab.py's:
  poisson  the 5-point matrix of an m x m grid (default m = 4096: 16.8 M rows, mean row length 5)
  banded   n = 2^20 rows, half-bandwidth 32 (65 entries per full row), SPD

Timing mode (default): a settle, then --rounds interleaved rounds; in each round every configuration -- the
cgx_create_csr context, and for each P in --blocks the indexed and the whole-slice context -- runs --iters fixed-count
iterations after a warm one, the order reversed every other round; ms per iteration by the host clock around a
synchronize.  One JSON line per round, then a summary per configuration: the median, the round-to-round spread
((max - min) / median), the entries each form moves per iteration (csr_halo() for the indexed one, P (n - n / P)
for the whole-slice one) and their bytes (12 per listed entry: the offset read and the value; 8 per whole-slice
entry).

Trace mode (--trace P): nothing is timed; the indexed and the whole-slice context over P blocks run --iters
iterations each, for `rocprofv3 --kernel-trace --stats` around this process: the exchange's own time is the average
of k_gather_indexed (indexed) and of k_gather_slices (whole slices) in its kernel statistics, P launches per
iteration each.

  python tools/csr_multi_ab.py --matrix poisson [--m 4096] [--blocks 1 2 4 8] [--out profiles/csr_multi_ab_poisson.jsonl]
  python tools/csr_multi_ab.py --matrix banded [--logn 20] [--hb 32]
  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/csr_multi_ab.py --matrix poisson --trace 8
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
from spmv_ab import banded_csr, poisson_csr  # noqa: E402


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def run(s, iters):
    """ms per iteration of `iters` fixed-count iterations after a warm one, host clock around a synchronize."""
    s.fill(1.0, 0.0)
    s.begin()
    s.iterate(1, eps=-1.0)
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
    ap.add_argument("--blocks", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--trace", type=int, default=0, metavar="P")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.matrix == "poisson":
        csr = poisson_csr(args.m)
        label = f"poisson m={args.m}"
    else:
        csr = banded_csr(1 << args.logn, args.hb)
        label = f"banded n=2^{args.logn} hb={args.hb}"
    n, nnz = csr[0].size - 1, int(csr[0][-1])
    if cg.device_count() < 1:
        sys.exit("no GPU visible: nothing is measured")

    def make(P, form):
        """The context over P blocks under the exchange form ("index" / "full"), or cgx_create_csr (P = 0)."""
        if P == 0:
            return cg.Solver.from_csr(*csr)
        os.environ["CGX_CSR_XCHG"] = form
        try:
            s = cg.Solver.from_csr(*csr, devices=[0] * P)
        finally:
            del os.environ["CGX_CSR_XCHG"]
        assert bool(s.info.flags & cg.CGX_CSR_HALO_ACTIVE) == (form == "index" and P > 1)
        return s

    if args.trace:
        for form in ("index", "full"):
            with make(args.trace, form) as s:
                run(s, args.iters)
        return

    out = args.out or os.path.join("profiles", f"csr_multi_ab_{args.matrix}.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    configs = [(0, "one")] + [(P, form) for P in args.blocks for form in (("index", "full") if P > 1 else ("index",))]
    ctx = {c: make(*c) for c in configs}
    with open(out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        moved = {}
        for (P, form), s in ctx.items():
            if P > 1:
                listed = int(s.csr_halo().sum())
                entries = listed if form == "index" else P * (n - n // P)
                moved[P, form] = {"entries_per_iteration": entries, "bytes_per_iteration": entries * (12 if form == "index" else 8),
                                  "largest_block_entries": int(s.csr_halo().sum(axis=1).max()) if form == "index" else n - n // P}
        emit({"record": "setup", "matrix": label, "n": n, "nnz": nnz, "rounds": args.rounds, "iters": args.iters,
              "devices": "every block on device 0", "plans": {f"{P},{form}": s.matvec_plan() for (P, form), s in ctx.items()}})
        t_end = time.perf_counter() + args.settle
        while True:
            for s in ctx.values():
                run(s, 2)
            if time.perf_counter() >= t_end:
                break
        ms = {c: [] for c in configs}
        for r in range(args.rounds):
            for c in (configs if r % 2 == 0 else configs[::-1]):
                ms[c].append(run(ctx[c], args.iters))
            emit({"record": "round", "round": r, "iteration_ms": {f"{P},{form}": round(ms[P, form][r], 5) for P, form in configs}})
        one = statistics.median(ms[0, "one"])
        for c in configs:
            med = statistics.median(ms[c])
            emit({"record": "summary", "matrix": label, "blocks": c[0], "form": c[1], "iteration_ms": round(med, 5),
                  "spread": round(spread(ms[c]), 5), "over_one_block": round(med / one, 4), **moved.get(c, {})})
    for s in ctx.values():
        s.close()


if __name__ == "__main__":
    main()
