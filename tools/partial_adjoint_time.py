"""Time Solver.factorAdjointUpTo (the reverse-mode sweep of a partial factor) beside factorAdjoint,
Solver.schurComplement beside a plain device copy of m^2 elements, and the forward / backward of
baspacho_amd.autograd.schur_complement, on BAL-871 (synthetic) cut at the end of its elimination
range, GRID 82x82 and one MERI problem cut at the root lump.  Events, warm-ups, median of --reps.  One
JSON line per problem and batch size.

    python tools/partial_adjoint_time.py [--reps 5] [--warmup 2] [--only bal871,grid82,meri] [--batch 0,8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from selinv_time import problems  # noqa: E402


def cut_span(sol):
    """the end of the elimination ranges where there are some, else the root lump"""
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    lump = ranges[-1] if ranges and ranges[-1] < sol.numLumps() else sol.numLumps() - 1
    return int(sol.skel()["lumpToSpan"][lump])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82,meri")
    ap.add_argument("--batch", default="0,8")
    a = ap.parse_args()
    import torch
    from baspacho_amd import autograd as BA
    from baspacho_amd import testing as T
    for name in a.only.split(","):
        sol = problems()[name]()
        span = cut_span(sol)
        m = sol.order() - int(sol.skel()["spanStart"][span])
        plan, full = sol._testSelInvPlan(span), sol._testSelInvPlan()
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        src = torch.from_numpy(h).to("cuda")
        for batch in (int(x) for x in a.batch.split(",")):
            nb = max(batch, 1)
            need = nb * (10 * sol.dataSize() + 4 * m * m) * 8
            free = torch.cuda.mem_get_info()[0]
            if need > 0.8 * free:
                print(json.dumps({"problem": name, "batch": batch, "skipped": "needs about %.0f GB, %.0f GB free"
                                  % (need / 1e9, free / 1e9)}), flush=True)
                continue
            sel = (lambda t: list(t.unbind(0))) if batch else (lambda t: t)
            L = src.repeat(nb, 1) if batch else src.clone()
            sol.factor(sel(L))
            P = src.repeat(nb, 1) if batch else src.clone()
            sol.factorUpTo(sel(P), span)
            pbar = torch.rand_like(P)
            dense = torch.empty((nb, m, m) if batch else (m, m), dtype=torch.float64, device="cuda")
            other = torch.empty_like(dense)
            W = torch.rand_like(dense)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
            t = {k: [] for k in ("up_to", "full", "dense", "copy", "fwd", "bwd")}
            for it in range(a.warmup + a.reps):
                g, g2 = pbar.clone(), pbar.clone()
                d = (src.repeat(nb, 1) if batch else src.clone()).requires_grad_(True)
                torch.cuda.synchronize()
                ev[0].record()
                sol.factorAdjointUpTo(sel(P), sel(g), span)
                ev[1].record()
                sol.factorAdjoint(sel(L), sel(g2))
                ev[2].record()
                sol.schurComplement(sel(P), span, out=sel(dense))
                ev[3].record()
                other.copy_(dense)
                ev[4].record()
                S = BA.schur_complement(sol, d, span)
                ev[5].record()
                (W * S).sum().backward()
                ev[6].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    for i, k in enumerate(("up_to", "full", "dense", "copy", "fwd", "bwd")):
                        t[k].append(ev[i].elapsed_time(ev[i + 1]))
            assert torch.isfinite(g).all().item() and torch.isfinite(d.grad).all().item()
            med = lambda v: round(float(np.median(v)), 3)
            print(json.dumps({
                "problem": name, "order": sol.order(), "cut_span": span, "schur_order": m, "batch": batch,
                "reps": a.reps, "plan_levels": plan["numLevels"], "full_plan_levels": full["numLevels"],
                "factor_adjoint_up_to_ms": med(t["up_to"]), "factor_adjoint_up_to_ms_min": round(float(np.min(t["up_to"])), 3),
                "factor_adjoint_ms": med(t["full"]), "factor_adjoint_ms_min": round(float(np.min(t["full"])), 3),
                "schur_to_dense_ms": med(t["dense"]), "dense_copy_ms": med(t["copy"]),
                "schur_over_copy": round(med(t["dense"]) / max(med(t["copy"]), 1e-6), 2),
                "schur_complement_forward_ms": med(t["fwd"]), "schur_complement_backward_ms": med(t["bwd"])}),
                flush=True)
            del L, P, pbar, dense, other, W, g, g2, d, S
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
