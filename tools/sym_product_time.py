"""Time the products with a matrix given as entries (baspacho_amd.sparse) in fp64,
with device events, warmed up, median of --reps; the routes of one problem are timed in one run, alternating.

  matvec at q = 1 and q = 10: SymProduct.mv against what the library offered before for A x from entries:
      Assembly.assemble into the layout, the vectors permuted to internal order and laid out as columns,
      Solver.addMvFrom from span 0 into zeroed columns, and the permutation back.  Both routes are checked
      against each other before anything is timed; the gradient kernel (outer) is timed beside them.
  solve_refined against sparse.solve in fp64, forward and forward + backward, and how far apart their
      results are.

Problems as in tools/assemble_time.py: the entries of the BAL-871 stand-in's Hessian and of GRID 82x82, every
element of every block of the input structure, without fill.  The rate of mv is its bytes over its event
time against the 6.29 TB/s HBM peak of the MI355X: it writes out and reads the row starts, per term the
entry index, the x index, one gathered value and q gathered elements of x.  One JSON line per problem.

The lines are printed and written to profiles/sym_product_time.txt (--out).

    python tools/sym_product_time.py [--reps 5] [--warmup 2] [--only grid82,bal871] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from assemble_time import HBM_TBPS, block_entries, problems  # noqa: E402


def timed_alternating(fns, warmup, reps):
    """median event time (ms) of every function of `fns`, one call of each per round"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {k: [] for k in fns}
    for it in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[k].append(a.elapsed_time(b))
    return {k: round(float(np.median(v)), 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,bal871")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sym_product_time.txt"),
                    help="the JSON lines go to this file as well (overwritten)")
    a = ap.parse_args()
    open(a.out, "w").close()
    import torch
    from baspacho_amd import sparse as S
    for name in a.only.split(","):
        sizes, ss = problems()[name]()
        rows, cols = block_entries(sizes, ss)
        n, nnz, sz = int(np.sum(sizes)), len(rows), 8
        pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes)
        t0 = time.perf_counter()
        prod = pat.product
        t_map = time.perf_counter() - t0
        sol, asm, info = pat.solver, pat.assembly, prod.info()
        rng = np.random.default_rng(37)
        vals = rng.uniform(-1.0, 1.0, nnz)
        vals[rows == cols] = n * 1.2  # diagonally dominant: the factor exists
        v = torch.from_numpy(vals).cuda()
        ds = sol.dataSize()
        rec = {"problem": name, "order": n, "nnz": nnz, "data_size": ds, "terms": info["terms"],
               "max_row": info["max_row"], "long_rows": info["long_rows"], "map_build_s": round(t_map, 2),
               "map_device_bytes": info["device_bytes"], "layout_bytes": ds * sz, "hbm_peak_tbps": HBM_TBPS}
        data = torch.empty(ds, dtype=torch.float64, device="cuda")
        to_int, to_user = pat._index("to_internal", v.device), pat._index("to_user", v.device)
        for q in (1, 10):
            x = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, q))).cuda()
            out = torch.empty_like(x)
            g = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, q))).cuda()
            gv = torch.empty_like(v)
            holder = {}

            def before():
                asm.assemble(v, out=data)
                xin = x.index_select(0, to_int).t().contiguous()  # [q, n]: columns in internal order
                y = torch.zeros_like(xin)
                sol.addMvFrom(data, 0, xin, n, y, n, nRHS=q)
                holder["y"] = y.t().index_select(0, to_user)

            def before_mv_only():  # the layout already assembled: what a loop over one matrix would pay
                xin = x.index_select(0, to_int).t().contiguous()
                y = torch.zeros_like(xin)
                sol.addMvFrom(data, 0, xin, n, y, n, nRHS=q)
                holder["y"] = y.t().index_select(0, to_user)

            before()
            prod.mv(v, x, out=out)
            scale = float(holder["y"].abs().max())
            rec["q%d_max_diff_rel" % q] = float((holder["y"] - out).abs().max()) / scale
            t = timed_alternating({"mv": lambda: prod.mv(v, x, out=out), "before": before,
                                   "before_mv_only": before_mv_only, "outer": lambda: prod.outer(g, x, out=gv)},
                                  a.warmup, a.reps)
            mv_bytes = n * q * sz + 4 * (n + 1) + info["terms"] * (8 + sz + q * sz)
            rec.update({"q%d_mv_ms" % q: t["mv"], "q%d_assemble_addmv_ms" % q: t["before"],
                        "q%d_addmv_only_ms" % q: t["before_mv_only"], "q%d_outer_ms" % q: t["outer"],
                        "q%d_mv_tbps" % q: round(mv_bytes / (t["mv"] * 1e9), 3)})
            del x, out, g, gv, holder
        del data
        torch.cuda.empty_cache()
        b = torch.randn(n, dtype=torch.float64, device="cuda")
        fns, holders = {}, {}
        for fname, fn in (("solve_refined", S.solve_refined), ("solve", S.solve)):
            vv, bb = v.clone().requires_grad_(True), b.clone().requires_grad_(True)
            holders[fname] = {}

            def fwd(fn=fn, vv=vv, bb=bb, h=holders[fname]):
                h["x"] = fn(pat, vv, bb)

            def fwd_bwd(fn=fn, vv=vv, bb=bb, h=holders[fname]):
                vv.grad = bb.grad = None
                h["x"] = fn(pat, vv, bb)
                h["x"].sum().backward()
                h["gv"], h["gb"] = vv.grad, bb.grad
            fns[fname + "_fwd_ms"], fns[fname + "_fwd_bwd_ms"] = fwd, fwd_bwd
        rec.update(timed_alternating(fns, a.warmup, a.reps))
        hr, hs = holders["solve_refined"], holders["solve"]
        for key in ("x", "gv", "gb"):
            rec["refined_vs_solve_%s_rel" % key] = float((hr[key] - hs[key]).abs().max()) / float(hs[key].abs().max())
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del pat, prod, sol, asm, v, holders, fns, hr, hs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
