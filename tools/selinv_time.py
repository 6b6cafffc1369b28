"""Time factor() + selectedInverse() on the device (events, warmed up, several repetitions) on BAL-871
(synthetic, point range [0, 527480]), GRID 82x82 and one MERI problem; prints one JSON line per problem.
Rates: selected inversion does 2 x bsp_factor_flops ("Selected inversion").
--batch N: N copies of the problem's factor instead, one batched selectedInverse(list) against N
single calls in a loop (each timed from a fresh batched factor, with the same events).

    python tools/selinv_time.py [--reps 5] [--warmup 2] [--only bal871,grid82,meri] [--batch N]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import baspacho_amd as B  # noqa: E402
from baspacho_amd import testing as T  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82,meri")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--batch", type=int, default=0)
    a = ap.parse_args()
    import torch
    dt = torch.float64 if a.dtype == "f64" else torch.float32
    for name in a.only.split(","):
        sol = problems()[name]()
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        src = torch.from_numpy(h).to("cuda", dt)
        if a.batch > 0:
            time_batch(sol, name, src, a)
            continue
        d = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        fac, inv = [], []
        for it in range(a.warmup + a.reps):
            d.copy_(src)
            ev[0].record()
            sol.factor(d)
            ev[1].record()
            sol.selectedInverse(d)
            ev[2].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                fac.append(ev[0].elapsed_time(ev[1]))
                inv.append(ev[1].elapsed_time(ev[2]))
        assert torch.isfinite(d).all().item()
        flops = 2.0 * sol.factorFlops()
        med = float(np.median(inv))
        print(json.dumps({
            "problem": name, "dtype": a.dtype, "order": sol.order(), "lumps": sol.numLumps(),
            "reps": a.reps, "factor_ms_median": round(float(np.median(fac)), 3),
            "selinv_ms_median": round(med, 3), "selinv_ms_min": round(float(np.min(inv)), 3),
            "selinv_ms_max": round(float(np.max(inv)), 3), "selinv_gflop": round(flops / 1e9, 2),
            "selinv_gflops_per_s": round(flops / (med * 1e6), 1),
            "selinv_over_factor": round(med / float(np.median(fac)), 2)}), flush=True)


def time_batch(sol, name, src, a):
    """one batched selectedInverse of `a.batch` factors against as many single calls"""
    import torch
    ds = [torch.empty_like(src) for _ in range(a.batch)]

    def fresh():
        for d in ds:
            d.copy_(src)
        sol.factor(ds)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    batched, loop = [], []
    c0 = sol.runCounters()
    for it in range(a.warmup + a.reps):
        fresh()
        ev[0].record()
        sol.selectedInverse(ds)
        ev[1].record()
        fresh()
        ev[2].record()
        for d in ds:
            sol.selectedInverse(d)
        ev[3].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            batched.append(ev[0].elapsed_time(ev[1]))
            loop.append(ev[2].elapsed_time(ev[3]))
    c1 = sol.runCounters()
    assert all(torch.isfinite(d).all().item() for d in ds)
    runs = a.warmup + a.reps
    mb, ml = float(np.median(batched)), float(np.median(loop))
    flops = 2.0 * sol.factorFlops() * a.batch
    print(json.dumps({
        "problem": name, "dtype": a.dtype, "batch": a.batch, "order": sol.order(), "reps": a.reps,
        "batched_ms_median": round(mb, 3), "batched_ms_min": round(float(np.min(batched)), 3),
        "batched_ms_max": round(float(np.max(batched)), 3), "loop_ms_median": round(ml, 3),
        "loop_ms_min": round(float(np.min(loop)), 3), "loop_ms_max": round(float(np.max(loop)), 3),
        "batched_ms_per_matrix": round(mb / a.batch, 3), "loop_over_batched": round(ml / mb, 2),
        "batched_gflops_per_s": round(flops / (mb * 1e6), 1),
        "chunks_per_batched_call": (c1["selinv_chunks"] - c0["selinv_chunks"] - runs * a.batch) / runs}),
        flush=True)


if __name__ == "__main__":
    main()
