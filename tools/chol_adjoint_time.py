"""Time Solver.factorAdjoint (the factor's reverse-mode sweep) beside selectedInverse on BAL-871
(synthetic, point range [0, 527480]), GRID 82x82 and one MERI problem, and the forward / backward of
x = L^-T z through baspacho_amd.autograd.cholesky + solve_lt (the core of sparse.sample, without
the assembly and the permutations).  One JSON line per problem and batch size.

    python tools/chol_adjoint_time.py [--reps 5] [--warmup 2] [--only bal871,grid82,meri] [--batch 0,8,64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from selinv_time import problems  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82,meri")
    ap.add_argument("--batch", default="0,8,64")
    a = ap.parse_args()
    import torch
    from baspacho_amd import autograd as BA
    from baspacho_amd import testing as T
    for name in a.only.split(","):
        sol = problems()[name]()
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        src = torch.from_numpy(h).to("cuda")
        for batch in (int(x) for x in a.batch.split(",")):
            nb = max(batch, 1)
            need = 10 * nb * sol.dataSize() * 8  # L, lbar, g, Z, d, its grad and the autograd clones
            free = torch.cuda.mem_get_info()[0]
            if need > 0.8 * free:
                print(json.dumps({"problem": name, "batch": batch, "skipped": "needs about %.0f GB, %.0f GB free"
                                  % (need / 1e9, free / 1e9)}), flush=True)
                continue
            L = src.repeat(nb, 1) if batch else src.clone()
            sol.factor(list(L.unbind(0)) if batch else L)
            lbar = torch.rand_like(L)
            z = torch.rand((nb, sol.order()) if batch else (sol.order(),), dtype=torch.float64, device="cuda")
            sel = (lambda t: list(t.unbind(0))) if batch else (lambda t: t)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            t_adj, t_inv, t_fwd, t_bwd = [], [], [], []
            for it in range(a.warmup + a.reps):
                g = lbar.clone()
                Z = L.clone()
                d = src.repeat(nb, 1) if batch else src.clone()
                d.requires_grad_(True)
                torch.cuda.synchronize()
                ev[0].record()
                sol.factorAdjoint(sel(L), sel(g))
                ev[1].record()
                sol.selectedInverse(sel(Z))
                ev[2].record()
                x = BA.solve_lt(sol, BA.cholesky(sol, d), z)
                ev[3].record()
                x.sum().backward()
                ev[4].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t_adj.append(ev[0].elapsed_time(ev[1]))
                    t_inv.append(ev[1].elapsed_time(ev[2]))
                    t_fwd.append(ev[2].elapsed_time(ev[3]))
                    t_bwd.append(ev[3].elapsed_time(ev[4]))
            assert torch.isfinite(g).all().item() and torch.isfinite(d.grad).all().item()
            med = lambda v: round(float(np.median(v)), 3)
            print(json.dumps({
                "problem": name, "order": sol.order(), "batch": batch, "reps": a.reps,
                "factor_adjoint_ms": med(t_adj), "factor_adjoint_ms_min": round(float(np.min(t_adj)), 3),
                "selected_inverse_ms": med(t_inv), "adjoint_over_selinv": round(med(t_adj) / med(t_inv), 2),
                "sample_forward_ms": med(t_fwd), "sample_backward_ms": med(t_bwd)}), flush=True)
            del L, lbar, z, g, Z, d, x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
