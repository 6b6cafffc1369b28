"""Time the autograd functions of baspacho_amd.autograd (forward and backward of solve, logdet and
solve_logdet) and their two kernels on their own (logDet; patternGrad write-only with U = V of one
right-hand side, and with Z read too), with device events, warmed up, median of --reps.  Problems as in
tools/selinv_time.py: BAL-871 (synthetic, point range [0, 527480]), GRID 82x82 and MERI; --batch N
runs GRID with a [N, dataSize] batch instead.  One JSON line per problem.  patternGrad's rate is its
bytes (dataSize x sizeof(T) written, as much again read with Z) over its event time, against the
6.29 TB/s HBM peak of the MI355X; kernel-only times come from a separate run of this tool under
`rocprofv3 --kernel-trace --stats`.

    python tools/autograd_time.py [--reps 5] [--warmup 2] [--only bal871,grid82,meri] [--batch N]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import baspacho_amd as B  # noqa: E402
from baspacho_amd import testing as T  # noqa: E402

HBM_TBPS = 6.29


def problems():
    def bal871():
        sizes, ss, _, _ = T.gen_bal_synthetic()
        return B.create_solver(B.Settings(), sizes, ss, [0, 527480])

    def grid82():
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
        return B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)

    def meri():
        ss = T.gen_meridians(4, 1500, 0.5, 120, 600, 2, 2, 37)
        return B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)

    return {"bal871": bal871, "grid82": grid82, "meri": meri}


def timed(fn, warmup, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82,meri")
    ap.add_argument("--batch", type=int, default=0)
    a = ap.parse_args()
    import torch
    from baspacho_amd import autograd as BA
    names = ["grid82"] if a.batch > 0 else a.only.split(",")
    for name in names:
        sol = problems()[name]()
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        src = torch.from_numpy(h).to("cuda")
        n, ds = sol.order(), sol.dataSize()
        if a.batch > 0:
            src = src[None].repeat(a.batch, 1)
        b = torch.randn(src.shape[:-1] + (n,), dtype=torch.float64, device="cuda")
        rec = {"problem": name, "batch": a.batch, "order": n, "data_bytes": ds * 8, "reps": a.reps}
        for fname in ("solve", "logdet", "solve_logdet"):
            d = src.clone().requires_grad_(True)
            bb = b.clone().requires_grad_(True)
            holder = {}

            def fwd():
                if fname == "solve":
                    holder["loss"] = BA.solve(sol, d, bb).sum()
                elif fname == "logdet":
                    holder["loss"] = BA.logdet(sol, d).sum()
                else:
                    x, ld = BA.solve_logdet(sol, d, bb)
                    holder["loss"] = x.sum() + ld.sum()

            def bwd():
                holder["loss"].backward(retain_graph=True)
            rec[fname + "_fwd_ms"] = timed(fwd, a.warmup, a.reps)
            rec[fname + "_bwd_ms"] = timed(bwd, a.warmup, a.reps)
            del holder
        if a.batch == 0:  # the kernels alone, on the factor of the problem
            L = src.clone()
            sol.factor(L)
            out = torch.empty_like(L)
            U = torch.randn((1, n), dtype=torch.float64, device="cuda")
            s = torch.ones(1, dtype=torch.float64, device="cuda")
            rec["logdet_kernel_ms"] = timed(lambda: sol.logDet(L), a.warmup, a.reps)
            t_uv = timed(lambda: sol.patternGrad(out, U=U, V=U, nRHS=1, alpha=-1.0), a.warmup, a.reps)
            t_z = timed(lambda: sol.patternGrad(out, Z=L, zScale=s), a.warmup, a.reps)
            rec["pattern_grad_uv_ms"] = t_uv
            rec["pattern_grad_z_ms"] = t_z
            rec["pattern_grad_uv_tbps"] = round(ds * 8 / (t_uv * 1e9), 3)
            rec["pattern_grad_z_tbps"] = round(2 * ds * 8 / (t_z * 1e9), 3)
            rec["hbm_peak_tbps"] = HBM_TBPS
            plain = src.clone()
            x = b.clone()
            rec["copy_factor_ms"] = timed(lambda: (plain.copy_(src), sol.factor(plain)), a.warmup, a.reps)
            rec["solve_ms"] = timed(lambda: sol.solve(plain, x, n, 1), a.warmup, a.reps)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
