"""Times the products with the factor (Solver.mulL / mulLt) beside the half-solves
(Solver.solveL / solveLt) on the same factor: the BAL-871 stand-in and GRID 82x82, fp64, nRHS = 1 and 10.

Every call is timed on its own with device events on the execution stream, after warm-up calls of the same
shape; the operations alternate inside one repetition so that they see the same machine.  Reported per
operation: the median, the fastest and the slowest call, and the bytes of L (the stored elements i >= j, each
read once by a product) per second of the median against the HBM bandwidth of the MI355X (8.0 TB/s peak,
about 6.3 TB/s achievable by a copy).  A half-solve reads the same bytes behind a dependency chain.  Needs a
GPU; prints one JSON line per workload and a table.

    python tools/factor_product_time.py [--reps 30] [--warmup 5] [--workloads bal871,grid82]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import baspacho_amd as B  # noqa: E402
from baspacho_amd import testing as T  # noqa: E402
from bench import build_problem  # noqa: E402

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3


def time_ops(sol, L, nrhs, reps, warmup):
    n = sol.order()
    x = torch.randn(nrhs, n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    v = torch.empty_like(x)
    ops = {"mulL": lambda: sol.mulL(L, x, out=y, nRHS=nrhs), "mulLt": lambda: sol.mulLt(L, x, out=y, nRHS=nrhs),
           "solveL": lambda: sol.solveL(L, v, nRHS=nrhs), "solveLt": lambda: sol.solveLt(L, v, nRHS=nrhs)}
    times = {k: [] for k in ops}
    for it in range(warmup + reps):
        for name, fn in ops.items():
            v.copy_(x)  # the solves work in place: a fresh right-hand side outside the timed window
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[name].append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workloads", default="bal871,grid82")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("factor_product_time.py needs a GPU: nothing is timed without one")
    rows = []
    for wl in args.workloads.split(","):
        sizes, ss, ranges, desc, _ = build_problem(wl)
        sol = B.create_solver(B.Settings(), sizes, ss, ranges)
        data = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(data, 0.0, sol.order() * 1.2)
        l_bytes = int(sol.lowerMask().sum()) * 8
        L = torch.from_numpy(data).cuda()
        sol.factor(L)
        torch.cuda.synchronize()
        for nrhs in (1, 10):
            times = time_ops(sol, L, nrhs, args.reps, args.warmup)
            rec = {"workload": desc, "order": sol.order(), "l_bytes": l_bytes, "nrhs": nrhs, "reps": args.reps}
            for name, ts in times.items():
                med = statistics.median(ts)
                rec[name] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts),
                             "l_tb_per_s": l_bytes / (med * 1e-3) / 1e12}
                rows.append((wl, nrhs, name, med, min(ts), max(ts), l_bytes / (med * 1e-3) / 1e12))
            print(json.dumps(rec), flush=True)
    print("\n| workload | nRHS | operation | median ms | min | max | bytes of L / s (TB/s) | of %.1f TB/s copy rate |"
          % HBM_COPY_TBS)
    print("|---|---|---|---|---|---|---|---|")
    for wl, nrhs, name, med, lo, hi, tbs in rows:
        print("| %s | %d | %s | %.3f | %.3f | %.3f | %.2f | %.0f %% |" % (wl, nrhs, name, med, lo, hi, tbs,
                                                                          100 * tbs / HBM_COPY_TBS))
    print("(HBM: %.1f TB/s peak, about %.1f TB/s achievable; nRHS = 10 reads L %d times in a product, once per "
          "group of 4 right-hand sides)" % (HBM_PEAK_TBS, HBM_COPY_TBS, 3))


if __name__ == "__main__":
    main()
