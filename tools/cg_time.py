"""Time the device-resident conjugate gradient of DESIGN.md section 24 in fp64, with device events, warmed up,
median of --reps; the routes of one comparison are timed in one run, alternating (tools/sym_product_time.py's
timer).

  solve_cg with every preconditioner (None, jacobi, block_jacobi, factor32) at a fixed number of iterations
      (tol = 0), for 10 and for 60 iterations, with check_every = 8 and None: the total, and the time of one
      more iteration = (t60 - t10) / 50.  That difference is an iteration's cost only while the columns run:
      with factor32 the residual reaches exactly 0 (or the iteration breaks down at rounding level) after a
      few steps, so its figures show what the steps behind a stop cost instead: nothing with check_every = 8
      (the queue ends), the product and the callable in full with check_every = None.  solve_cg's factor32
      totals include assembling and factoring the fp32 layout; the loop is handed a finished factor.
  pcg.PCG, the caller-side loop, given the same operator (SymProduct.mv) and the same kind of preconditioner
      as callables (None, a torch Jacobi, the fp32 factor), the same way.
  S.solve and S.solve_refined (3 corrections) on the same matrix and right-hand side, and solve_cg to
      tol = 1e-10 with its iteration counts.

Problems as in tools/assemble_time.py: GRID 82x82 and the BAL-871 stand-in, every element of every block of
the input structure, without fill; the off-diagonal values are uniform in (-1, 1) and the diagonal is 1.05
times the absolute row sum plus 0.1, so the matrix is positive definite without being nearly diagonal.  One
JSON line per problem, printed and written to profiles/cg_time.txt (--out).  launches_per_iteration is counted
from the launch sequence of section 24 (the product, two per dot product, the fused updates), not traced.

    python tools/cg_time.py [--reps 5] [--warmup 2] [--only grid82,bal871] [--out FILE]

--fsai: the "fsai" preconditioner of section 27 instead (default --out profiles/cg_fsai_time.txt), on the same
structures with two sets of values: "dominant", the generator above, and "ill", where every off-diagonal block
of the structure is an edge that adds Q = W^T W (W uniform in (0.2, 1)) to both diagonal blocks and -Q between
them, plus --shift times I (params of one size only).  Per problem and generator: the host time of the plan and
its sizes; the build of every built-in kind; one application of "block_jacobi" and of "fsai" beside one product
A p (50 calls between two events, in one process); and solve_cg to tol = 1e-10 with none / jacobi / block_jacobi
/ fsai: the time and the iterations.  A plan whose item count does not fit is reported with the count it states.
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

LAUNCHES = {"none": 6, "jacobi": 8, "block_jacobi": 8, "factor32": "7 + the fp32 solve's and its permutations'"}


def dominant_values(rows, cols, n, rng):
    """off-diagonal values uniform in (-1, 1), the diagonal 1.05 times the absolute row sum plus 0.1"""
    vals = rng.uniform(-1.0, 1.0, len(rows))
    off = rows != cols
    rowsum = np.zeros(n)
    np.add.at(rowsum, rows[off], np.abs(vals[off]))
    np.add.at(rowsum, cols[off], np.abs(vals[off]))
    vals[~off] = 1.05 * rowsum[rows[~off]] + 0.1
    return vals


def ill_values(sizes, ss, rows, cols, n, rng, shift):
    """every off-diagonal block (p, q) of the structure adds Q = W^T W to the diagonal blocks of p and q and -Q
    to the block between them; shift * I at the end.  Params of one size"""
    bs = int(sizes[0])
    assert (np.asarray(sizes) == bs).all(), "the ill-conditioned generator takes params of one size"
    starts = np.concatenate([[0], np.cumsum(sizes)])
    br = np.repeat(np.arange(len(sizes)), np.diff(ss.ptrs))
    bc = np.asarray(ss.inds, dtype=np.int64)
    sel = br != bc
    p, q = np.maximum(br[sel], bc[sel]), np.minimum(br[sel], bc[sel])
    W = rng.uniform(0.2, 1.0, (len(p), bs, bs))
    Q = np.einsum("eki,ekj->eij", W, W)
    lr, lc = np.meshgrid(np.arange(bs), np.arange(bs), indexing="ij")
    low = lr >= lc
    coo_r = np.concatenate([(starts[p][:, None, None] + lr[None]).ravel(),
                            (starts[p][:, None] + lr[low][None]).ravel(), (starts[q][:, None] + lr[low][None]).ravel()])
    coo_c = np.concatenate([(starts[q][:, None, None] + lc[None]).ravel(),
                            (starts[p][:, None] + lc[low][None]).ravel(), (starts[q][:, None] + lc[low][None]).ravel()])
    coo_v = np.concatenate([-Q.ravel(), Q[:, low].ravel(), Q[:, low].ravel()])
    key = rows * n + cols
    order = np.argsort(key, kind="stable")
    at = order[np.searchsorted(key[order], coo_r * n + coo_c)]
    assert (rows[at] == coo_r).all() and (cols[at] == coo_c).all()
    vals = np.zeros(len(rows))
    np.add.at(vals, at, coo_v)
    vals[rows == cols] += shift
    return vals


def fsai_main(a):
    """the measurements of DESIGN.md section 27"""
    import time
    import torch
    from baspacho_amd import cg as CG
    from baspacho_amd import sparse as S
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def per_call(fn, calls=50):
        """median over the reps of the event time of `calls` queued calls, per call (ms)"""
        ts = []
        for it in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(calls):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ts.append(ev[0].elapsed_time(ev[1]) / calls)
        return round(float(np.median(ts)), 5)

    for name in a.only.split(","):
        sizes, ss = problems()[name]()
        rows, cols = block_entries(sizes, ss)
        n, nnz = int(np.sum(sizes)), len(rows)
        pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes)
        prod, sol = pat.product, pat.solver
        base = {"problem": name, "order": n, "nnz": nnz, "terms": prod.info()["terms"], "reps": a.reps,
                "warmup": a.warmup, "launches_per_iteration": dict(LAUNCHES, fsai=9)}
        t0 = time.perf_counter()
        try:
            info = prod.cgFsaiTable()["info"]
        except RuntimeError as e:
            base["fsai_plan"] = str(e)
            info = None
        base["fsai_plan_host_s"] = round(time.perf_counter() - t0, 3)
        if info is not None:
            base["fsai_plan"] = info
        kinds = ["none", "jacobi"] + (["block_jacobi"] if int(np.max(sizes)) <= 32 else []) + (["fsai"] if info else [])
        gens = ["dominant"] + (["ill"] if len(set(np.asarray(sizes).tolist())) == 1 else [])
        for gen in gens:
            rng = np.random.default_rng(37)
            vals = dominant_values(rows, cols, n, rng) if gen == "dominant" else \
                ill_values(sizes, ss, rows, cols, n, rng, a.shift)
            v = torch.from_numpy(vals).cuda()
            b = torch.from_numpy(rng.uniform(-1.0, 1.0, n)).cuda()
            rec = dict(base, generator=gen, shift=a.shift if gen == "ill" else None)
            p1, ap = b.reshape(n, 1).clone(), torch.zeros(n, 1, dtype=b.dtype, device=b.device)
            rec["mv_ms"] = per_call(lambda: prod.mv(v, p1, out=ap))
            for kind in kinds[1:]:
                rec["build_%s_ms" % kind] = per_call(lambda kind=kind: CG.Preconditioner(prod, kind, v), calls=1)
            for kind in kinds[2:]:
                pc = CG.Preconditioner(prod, kind, v)
                run = CG.CgRun(sol, p1, torch.zeros_like(p1), p1.clone(), lambda p, out: prod.mv(v, p, out=out), pc, 0.0, 10)
                run.start()
                rec["apply_%s_ms" % kind] = per_call(run._apply_precond)
                rec["status_%s" % kind] = pc.status.tolist()
            h = {}
            fns = {k: (lambda k=k: h.__setitem__(k, S.solve_cg(pat, v, b, precond=None if k == "none" else k, tol=1e-10,
                                                              max_steps=a.max_steps, return_info=True))) for k in kinds}
            tm = timed_alternating(fns, a.warmup, a.reps)
            for k in kinds:
                x, i = h[k]
                rec["cg_tol_%s" % k] = {"ms": tm[k], "iterations": int(i["iterations"]), "stop": int(i["stop"]),
                                        "relres": float(i["relres"]),
                                        "true_relres": float((b - prod.mv(v, x)).norm() / b.norm())}
            line = json.dumps(rec)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            del v, b, h, fns
        del pat, prod, sol
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,bal871")
    ap.add_argument("--fsai", action="store_true", help="the measurements of the fsai preconditioner (section 27)")
    ap.add_argument("--shift", type=float, default=1e-3, help="--fsai: the shift of the ill-conditioned generator")
    ap.add_argument("--max-steps", type=int, default=5000, help="--fsai: the step limit of the solves to tol")
    ap.add_argument("--out", default=None, help="the JSON lines go to this file as well (overwritten); default "
                    "profiles/cg_time.txt, with --fsai profiles/cg_fsai_time.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "cg_fsai_time.txt" if a.fsai else "cg_time.txt")
    open(a.out, "w").close()
    if a.fsai:
        return fsai_main(a)
    import torch
    from baspacho_amd import autograd as ag
    from baspacho_amd import pcg
    from baspacho_amd import sparse as S
    for name in a.only.split(","):
        sizes, ss = problems()[name]()
        rows, cols = block_entries(sizes, ss)
        n, nnz = int(np.sum(sizes)), len(rows)
        pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes)
        prod, sol = pat.product, pat.solver
        rng = np.random.default_rng(37)
        vals = rng.uniform(-1.0, 1.0, nnz)
        off = rows != cols
        rowsum = np.zeros(n)
        np.add.at(rowsum, rows[off], np.abs(vals[off]))
        np.add.at(rowsum, cols[off], np.abs(vals[off]))
        vals[~off] = 1.05 * rowsum[rows[~off]] + 0.1
        v = torch.from_numpy(vals).cuda()
        b = torch.from_numpy(rng.uniform(-1.0, 1.0, n)).cuda()
        rec = {"problem": name, "order": n, "nnz": nnz, "terms": prod.info()["terms"], "max_param": int(np.max(sizes)),
               "reps": a.reps, "warmup": a.warmup, "launches_per_iteration": LAUNCHES}

        # ---- the caller-side loop's operator and preconditioners
        L32 = pat.assembly.assemble(v.float())
        sol.factor(L32)
        inv_diag = 1.0 / torch.from_numpy(vals[~off][np.argsort(rows[~off])]).cuda()

        def solve32(r):
            rt = ag._to_cols(pat.toInternal(r.float(), 0), False)
            ag._solve_cols(sol, L32, rt)
            return pat.fromInternal(ag._from_cols(rt, r.shape), 0).double()

        loop_m = {"none": pcg.IdentityPrecond(), "jacobi": lambda r: r * inv_diag, "factor32": solve32}
        fns, h = {}, {}
        for pc in ("none", "jacobi", "block_jacobi", "factor32"):
            if pc == "block_jacobi" and int(np.max(sizes)) > 32:
                rec["block_jacobi"] = "a param is wider than 32"
                continue
            arg = None if pc == "none" else pc
            for steps in (10, 60):
                for ce in (8, None):
                    key = "cg_%s_%d_ce%s" % (pc, steps, ce)
                    fns[key] = (lambda arg=arg, steps=steps, ce=ce, key=key: h.__setitem__(
                        key, S.solve_cg(pat, v, b, precond=arg, tol=0.0, max_steps=steps, check_every=ce)))
                if pc in loop_m:
                    key = "loop_%s_%d" % (pc, steps)
                    fns[key] = (lambda pc=pc, steps=steps: pcg.PCG(loop_m[pc], lambda p: prod.mv(v, p), 0.0, steps)
                                .solve(torch.empty_like(b), b))
        tm = timed_alternating(fns, a.warmup, a.reps)
        rec.update({k + "_ms": t for k, t in tm.items()})
        for k in list(tm):
            if "_60" in k:
                rec[k.replace("_60", "_per_iteration") + "_ms"] = round((tm[k] - tm[k.replace("_60", "_10")]) / 50.0, 5)

        # ---- to a tolerance, beside the direct solves
        b3 = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 3))).cuda()
        fns = {"solve": lambda: h.__setitem__("solve", S.solve(pat, v, b3)),
               "solve_refined": lambda: h.__setitem__("refined", S.solve_refined(pat, v, b3))}
        for pc in ("none", "jacobi", "block_jacobi", "factor32"):
            if pc == "block_jacobi" and int(np.max(sizes)) > 32:
                continue
            fns["cg_tol_" + pc] = (lambda pc=pc: h.__setitem__(pc, S.solve_cg(
                pat, v, b3, precond=None if pc == "none" else pc, tol=1e-10, max_steps=500, return_info=True)))
        tm = timed_alternating(fns, a.warmup, a.reps)
        rec.update({k + "_ms": t for k, t in tm.items()})
        ref = h["solve"]
        for pc in ("none", "jacobi", "block_jacobi", "factor32"):
            if pc in h:
                x, info = h[pc]
                rec["cg_tol_%s_iterations" % pc] = info["iterations"].tolist()
                rec["cg_tol_%s_stop" % pc] = info["stop"].tolist()
                rec["cg_tol_%s_diff_to_solve" % pc] = float((x - ref).norm() / ref.norm())
        rec["refined_diff_to_solve"] = float((h["refined"] - ref).norm() / ref.norm())
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del pat, prod, sol, v, b, b3, h, fns, L32
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
