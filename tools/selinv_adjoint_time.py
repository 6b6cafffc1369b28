"""Time Solver.selectedInverseAdjoint (the reverse mode of selected inversion) beside selectedInverse and
factorAdjoint of the same run on BAL-871 (synthetic, point range [0, 527480]), GRID 82x82 and one MERI
problem, single calls and batches, and the forward / backward of sparse.covariance on the entries of
the problem's own block pattern (problems with at most --max-entries entries: the host map of the
assembly is built entry by entry).  One JSON line per problem and batch size.

    python tools/selinv_adjoint_time.py [--reps 5] [--warmup 2] [--only bal871,grid82,meri] [--batch 0,8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import baspacho_amd as B  # noqa: E402
from baspacho_amd import testing as T  # noqa: E402


def structures():
    """name -> (param sizes, block structure, sparse elimination ranges)"""
    def bal871():
        sizes, ss, _, _ = T.gen_bal_synthetic()
        return sizes, ss, [0, 527480]

    def grid82():
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
        return np.full(ss.order(), 3, dtype=np.int64), ss, []

    def meri():
        ss = T.gen_meridians(4, 1500, 0.5, 120, 600, 2, 2, 37)
        return np.full(ss.order(), 3, dtype=np.int64), ss, []

    return {"bal871": bal871, "grid82": grid82, "meri": meri}


def entries(sizes, ss):
    """(rows, cols) of every scalar of the lower blocks of `ss`, row >= col"""
    st = np.concatenate([[0], np.cumsum(sizes)])
    p = np.repeat(np.arange(ss.order(), dtype=np.int64), np.diff(ss.ptrs))
    q = ss.inds
    rows, cols = [], []
    for sp, sq in {(int(x), int(y)) for x, y in zip(sizes[p], sizes[q])}:
        pick = (sizes[p] == sp) & (sizes[q] == sq)
        i = st[p[pick]][:, None, None] + np.arange(sp)[None, :, None] + np.zeros((1, 1, sq), dtype=np.int64)
        j = st[q[pick]][:, None, None] + np.arange(sq)[None, None, :] + np.zeros((1, sp, 1), dtype=np.int64)
        keep = i >= j
        rows.append(i[keep])
        cols.append(j[keep])
    return np.concatenate(rows), np.concatenate(cols)


def num_entries(sizes, ss):
    p = np.repeat(np.arange(ss.order(), dtype=np.int64), np.diff(ss.ptrs))
    return int((sizes[p] * sizes[ss.inds]).sum())


def med(v):
    return round(float(np.median(v)), 3)


def time_covariance(name, sizes, ss, a):
    import torch
    from baspacho_amd import sparse as S
    num = num_entries(sizes, ss)
    if num > a.max_entries:
        return {"covariance": "skipped: %d entries" % num}
    rows, cols = entries(sizes, ss)
    pat = S.SymmetricPattern(rows, cols, int(sizes.sum()), param_sizes=sizes)
    rng = np.random.default_rng(37)
    v = rng.uniform(-1, 1, len(rows))
    v[rows == cols] = 1.2 * pat.n
    vd = torch.from_numpy(v).to("cuda").requires_grad_(True)
    w = torch.rand(len(rows), dtype=torch.float64, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    fwd, bwd = [], []
    for it in range(a.warmup + a.reps):
        vd.grad = None
        torch.cuda.synchronize()
        ev[0].record()
        c = S.covariance(pat, vd)
        ev[1].record()
        (w * c).sum().backward()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            fwd.append(ev[0].elapsed_time(ev[1]))
            bwd.append(ev[1].elapsed_time(ev[2]))
    assert torch.isfinite(vd.grad).all().item()
    return {"covariance_entries": len(rows), "covariance_forward_ms": med(fwd), "covariance_backward_ms": med(bwd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82,meri")
    ap.add_argument("--batch", default="0,8")
    ap.add_argument("--max-entries", type=int, default=6000000)
    a = ap.parse_args()
    import torch
    for name in a.only.split(","):
        sizes, ss, ranges = structures()[name]()
        sol = B.create_solver(B.Settings(), sizes, ss, ranges) if ranges else B.create_solver(B.Settings(), sizes, ss)
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        src = torch.from_numpy(h).to("cuda")
        for batch in (int(x) for x in a.batch.split(",")):
            nb = max(batch, 1)
            need = 6 * nb * sol.dataSize() * 8  # L, Z, the gradient, its clone, the factor adjoint's buffer
            free = torch.cuda.mem_get_info()[0]
            if need > 0.8 * free:
                print(json.dumps({"problem": name, "batch": batch, "skipped": "needs about %.0f GB, %.0f GB free"
                                  % (need / 1e9, free / 1e9)}), flush=True)
                continue
            sel = (lambda t: list(t.unbind(0))) if batch else (lambda t: t)
            L = src.repeat(nb, 1) if batch else src.clone()
            sol.factor(sel(L))
            gz = torch.rand_like(L)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            t_inv, t_adj, t_fac = [], [], []
            for it in range(a.warmup + a.reps):
                Z = L.clone()
                g = gz.clone()
                torch.cuda.synchronize()
                ev[0].record()
                sol.selectedInverse(sel(Z))
                ev[1].record()
                sol.selectedInverseAdjoint(sel(L), sel(Z), sel(g))
                ev[2].record()
                sol.factorAdjoint(sel(L), sel(g))
                ev[3].record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t_inv.append(ev[0].elapsed_time(ev[1]))
                    t_adj.append(ev[1].elapsed_time(ev[2]))
                    t_fac.append(ev[2].elapsed_time(ev[3]))
            assert torch.isfinite(g).all().item()
            out = {"problem": name, "order": sol.order(), "batch": batch, "reps": a.reps,
                   "selected_inverse_ms": med(t_inv), "selected_inverse_adjoint_ms": med(t_adj),
                   "selected_inverse_adjoint_ms_min": round(float(np.min(t_adj)), 3),
                   "factor_adjoint_ms": med(t_fac), "adjoint_over_selinv": round(med(t_adj) / med(t_inv), 2)}
            del L, Z, g, gz
            torch.cuda.empty_cache()
            if batch == 0:
                out.update(time_covariance(name, sizes, ss, a))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
