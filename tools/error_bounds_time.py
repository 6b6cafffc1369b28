"""Time the error bounds of DESIGN.md section 23 in fp64, with device events, warmed up, median of --reps; the
routes of one comparison are timed in one run, alternating (tools/sym_product_time.py's timer).

  residual: SymProduct.residual (r and d in one pass) against the routes the library offered before:
      mv plus the torch subtraction (r alone), and those plus a separate absMv and |b| added (r and d);
      maxRatio of the pair beside them.
  invNorm1 and cond_estimate (plain and scaled) against one factor() and one solve() with one right-hand
      side on the same matrix.
  solve_refined with tol = 1e-14 (iters = 3 and iters = 6) and with return_info against the fixed three
      corrections, with the corrections each column took.

Problems as in tools/assemble_time.py: GRID 82x82 and the BAL-871 stand-in, every element of every block of
the input structure, without fill.  One JSON line per problem, printed and written to
profiles/error_bounds_time.txt (--out).

    python tools/error_bounds_time.py [--reps 5] [--warmup 2] [--only grid82,bal871] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from assemble_time import block_entries, problems  # noqa: E402
from sym_product_time import timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,bal871")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_bounds_time.txt"),
                    help="the JSON lines go to this file as well (overwritten)")
    a = ap.parse_args()
    open(a.out, "w").close()
    import torch
    from baspacho_amd import sparse as S
    for name in a.only.split(","):
        sizes, ss = problems()[name]()
        rows, cols = block_entries(sizes, ss)
        n, nnz = int(np.sum(sizes)), len(rows)
        pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes)
        prod, sol, asm = pat.product, pat.solver, pat.assembly
        rng = np.random.default_rng(37)
        vals = rng.uniform(-1.0, 1.0, nnz)
        vals[rows == cols] = n * 1.2  # diagonally dominant: the factor exists
        v = torch.from_numpy(vals).cuda()
        rec = {"problem": name, "order": n, "nnz": nnz, "terms": prod.info()["terms"],
               "long_rows": prod.info()["long_rows"], "reps": a.reps, "warmup": a.warmup}

        # ---- residual against the earlier routes
        for q in (1, 10):
            x = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, q))).cuda()
            b = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, q))).cuda()
            r, d, y, t = (torch.empty_like(x) for _ in range(4))
            h = {}

            def mv_sub():
                prod.mv(v, x, out=y)
                h["r"] = b - y

            def mv_sub_absmv():
                prod.mv(v, x, out=y)
                h["r"] = b - y
                prod.absMv(v, x, out=t)
                h["d"] = b.abs() + t

            prod.residual(v, x, b, out=(r, d))
            mv_sub_absmv()
            assert torch.equal(h["r"], r) and torch.equal(h["d"], d), "the routes disagree"
            tm = timed_alternating({"residual": lambda: prod.residual(v, x, b, out=(r, d)), "mv_sub": mv_sub,
                                    "mv_sub_absmv": mv_sub_absmv, "mv": lambda: prod.mv(v, x, out=y),
                                    "max_ratio": lambda: sol.maxRatio(r, d)}, a.warmup, a.reps)
            rec.update({"q%d_%s_ms" % (q, k): t_ for k, t_ in tm.items()})
            del x, b, r, d, y, t, h

        # ---- the estimate against one factor and one solve
        data = asm.assemble(v)
        L = data.clone()
        sol.factor(L)
        rhs = torch.ones(1, n, dtype=torch.float64, device="cuda")
        h = {}

        def factor():
            L.copy_(data)
            sol.factor(L)

        def copy_only():
            L.copy_(data)

        def inv_norm1():
            h["inv"] = sol.invNorm1(L)

        tm = timed_alternating({"copy_only": copy_only, "factor_with_copy": factor,
                                "solve_1rhs": lambda: sol.solve(L, rhs, stride=n, nRHS=1), "inv_norm1": inv_norm1,
                                "norm1": lambda: S.norm1(pat, v),
                                "cond_estimate": lambda: h.__setitem__("k", S.cond_estimate(pat, v)),
                                "cond_estimate_scaled": lambda: h.__setitem__("ks", S.cond_estimate(pat, v, scaled=True))},
                               a.warmup, a.reps)
        rec.update({k + "_ms": t_ for k, t_ in tm.items()})
        rec.update({"inv_norm1": float(h["inv"]), "cond_estimate": float(h["k"]), "cond_estimate_scaled": float(h["ks"])})
        st = sol.readNormEstState(sol.invNorm1(L, return_state=True)[1])
        rec.update({"inv_norm1_passes": st["passes"], "inv_norm1_stop": st["stopReason"]})
        del data, L, rhs

        # ---- checked refinement against the fixed three corrections
        b = torch.randn(n, 3, dtype=torch.float64, device="cuda")
        h = {}
        fns = {"refined_fixed3": lambda: h.__setitem__("x", S.solve_refined(pat, v, b)),
               "refined_tol_iters3": lambda: S.solve_refined(pat, v, b, iters=3, tol=1e-14),
               "refined_tol_iters6": lambda: S.solve_refined(pat, v, b, iters=6, tol=1e-14),
               "refined_fixed3_info": lambda: h.__setitem__("i", S.solve_refined(pat, v, b, return_info=True)[1]),
               "refined_tol_iters6_info": lambda: h.__setitem__(
                   "t", S.solve_refined(pat, v, b, iters=6, tol=1e-14, return_info=True)[1])}
        tm = timed_alternating(fns, a.warmup, a.reps)
        rec.update({k + "_ms": t_ for k, t_ in tm.items()})
        rec.update({"fixed3_berr_max": float(h["i"]["berr"].max()), "tol_berr_max": float(h["t"]["berr"].max()),
                    "tol_corrections": h["t"]["corrections"].tolist()})
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del pat, prod, sol, asm, v, b, h, fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
