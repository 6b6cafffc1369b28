"""Time the matrix-free least squares of DESIGN.md section 28 in fp64, with device events, warmed up, median of
--reps with the lowest and highest repetition beside it; the routes of one comparison are timed in one process,
alternating (tools/cg_time.py's protocol).

  J^T u and J v (q = 1) through the JacobianOperator's lists (a wave for a run of more than 64 entries) against
      jtVec / jVec of the JacobianPattern (one lane per run): the time, the bytes moved (the output, the run
      starts, entry and gathered index per term, the value and the gathered operand per term) and their share of
      the 6.29 TB/s HBM peak.
  One iteration with 3 right-hand sides = (t60 - t10) / 50 at tol = 0, and the solve to tol = 1e-10:
      sparse.lstsq_cg (none / jacobi / block_jacobi), the composed route (cg.CgRun given the callable p -> J^T (J
      p) + d p built from the pattern's jVec / jtVec, with no preconditioner and with a torch Jacobi), and
      sparse.lstsq (the factor) for the solve.
  The attained accuracy of CGLS and of the composed CG against a dense QR solution on one ill-conditioned
      Jacobian (kappa(J) about 1e6 by column scaling, no preconditioner, no damping).
  The host build time and the device bytes of the operator's map and plan against the JacobianPattern's maps, and
      the bytes computed (not measured) for the BAL-871 stand-in from its counts.

Problems: tools/normal_eq_time.py's (the GRID 82x82 pose graph and the small BAL shape).  One JSON line per
problem, printed and written to profiles/cgls_time.txt (--out).

    python tools/cgls_time.py [--reps 5] [--warmup 2] [--only grid82,balsmall] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from assemble_time import HBM_TBPS  # noqa: E402
from normal_eq_time import problems  # noqa: E402

LAUNCHES = {"none": "7, one call", "jacobi": "7, one call", "block_jacobi": "7, one call",
            "composed": "8 without a preconditioner (jVec, jtVec, the torch addcmul, 5 of CgRun), 11 with the torch Jacobi"}
DAMPING = (1e-3, 1e-3)


def timed_alternating(fns, warmup, reps):
    """{name: (median, lowest, highest)} event time (ms) of every function of `fns`, one call of each per round"""
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
    return {k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for k, v in out.items()}


def composed_cg(jpat, v, r3, d, jacobi, tol, max_steps, check_every=8):
    """the parent's capability: CG on the formed operator p -> J^T (J p) + d p, the residual kept in n-space"""
    import torch
    from baspacho_amd import cg as CG
    ne = jpat.normal_eq
    b = ne.jtVec(v, r3)
    t = torch.empty_like(r3)

    def apply_a(p, ap):
        ne.jVec(v, p, out=t)
        ne.jtVec(v, t, out=ap)
        ap.addcmul_(d[:, None], p)
        return ap

    pc = None if jacobi is None else (lambda s: s * jacobi[:, None])
    x = torch.zeros_like(b)
    run = CG.CgRun(jpat.solver, b, x, b.clone(), apply_a, pc, tol, max_steps).run(check_every)
    return x, run


def ill_conditioned(a):
    """CGLS and the composed CG on J = J0 diag(10^(-6 i / n)): what each attains against the QR solution"""
    import torch
    from baspacho_amd import sparse as S
    rng = np.random.default_rng(41)
    m, n = 600, 200
    sets = [rng.choice(n, 4, replace=False) for _ in range(m - n)]
    rows = np.concatenate([np.repeat(np.arange(m - n), 4), m - n + np.arange(n)])
    cols = np.concatenate([np.concatenate(sets), np.arange(n)])
    scale = 10.0 ** (-6.0 * np.arange(n) / (n - 1))
    vals = np.concatenate([rng.uniform(-1, 1, 4 * (m - n)), np.full(n, 2.0)]) * scale[cols]
    J = np.zeros((m, n))
    J[rows, cols] = vals
    r = rng.uniform(-1, 1, (m, 1))
    xq = np.linalg.lstsq(J, r, rcond=None)[0]
    jpat = S.JacobianPattern(rows, cols, m, n)
    v, rd = torch.from_numpy(vals).cuda(), torch.from_numpy(r).cuda()
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = {"m": m, "n": n, "kappa_J": float(np.linalg.cond(J)), "max_steps": a.ill_steps}
    x, info = S.lstsq_cg(jpat, v, rd, precond=None, tol=1e-15, max_steps=a.ill_steps, return_info=True)
    xc, run = composed_cg(jpat, v, rd, zero, None, 1e-15, a.ill_steps)
    for name, xx, its, stop in (("cgls", x, info["iterations"], info["stop"]), ("composed_cg", xc, run.iterations(), run.stop())):
        xx = xx.cpu().numpy()
        out[name] = {"iterations": int(its), "stop": int(stop),
                     "error_vs_qr": float(np.linalg.norm(xx - xq) / np.linalg.norm(xq)),
                     "normal_residual": float(np.linalg.norm(J.T @ (r - J @ xx)) / np.linalg.norm(J.T @ r))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,balsmall")
    ap.add_argument("--ill-steps", type=int, default=4000, help="the step limit on the ill-conditioned Jacobian")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cgls_time.txt"),
                    help="the JSON lines go to this file as well (overwritten)")
    a = ap.parse_args()
    open(a.out, "w").close()
    import torch
    from baspacho_amd import cgls as CGLS
    from baspacho_amd import sparse as S
    emit = lambda rec: (print(json.dumps(rec), flush=True), open(a.out, "a").write(json.dumps(rec) + "\n"))
    for name in a.only.split(","):
        sizes, (rows, cols, vals, m, n) = problems()[name]()
        nnz, sz = len(rows), 8
        t0 = time.perf_counter()
        op = S.JacobianOperator(rows, cols, m, n, param_sizes=sizes)
        t_op = time.perf_counter() - t0
        t0 = time.perf_counter()
        plan = op.product.precondInfo("block_jacobi")
        t_plan = time.perf_counter() - t0
        t0 = time.perf_counter()
        jpat = S.JacobianPattern(rows, cols, m, n, param_sizes=sizes)
        t_pat = time.perf_counter() - t0
        oi, pi = op.product.info(), jpat.normal_eq.info()
        rec = {"problem": name, "m": m, "order": n, "nnz": nnz, "reps": a.reps, "warmup": a.warmup,
               "hbm_peak_tbps": HBM_TBPS, "launches_per_iteration": LAUNCHES, "damping": DAMPING,
               "operator": {"host_build_s": round(t_op, 3), "plan_host_s": round(t_plan, 3), "row_bytes": oi["row_bytes"],
                            "col_bytes": oi["col_bytes"], "plan_bytes": plan["device_bytes"], "plan_items": plan["items"],
                            "max_row": oi["max_row"], "long_rows": oi["long_rows"], "max_col": oi["max_col"],
                            "long_cols": oi["long_cols"]},
               "pattern": {"host_build_s": round(t_pat, 3), "pairs": pi["pairs"], "forward_bytes": pi["forward_bytes"],
                           "adjoint_bytes": pi["adjoint_bytes"], "vector_bytes": pi["vector_bytes"]}}
        v = torch.from_numpy(vals).cuda()
        rng = np.random.default_rng(37)
        u1, w1 = torch.from_numpy(rng.uniform(-1, 1, m)).cuda(), torch.from_numpy(rng.uniform(-1, 1, n)).cuda()
        g1, y1 = torch.empty_like(w1), torch.empty_like(u1)
        ne, pr = jpat.normal_eq, op.product
        assert torch.equal(pr.jtVec(v, u1), ne.jtVec(v, u1)) and torch.equal(pr.jVec(v, w1), ne.jVec(v, w1))
        tm = timed_alternating({"jt_operator": lambda: pr.jtVec(v, u1, out=g1), "jt_pattern": lambda: ne.jtVec(v, u1, out=g1),
                                "jv_operator": lambda: pr.jVec(v, w1, out=y1), "jv_pattern": lambda: ne.jVec(v, w1, out=y1)},
                               a.warmup, a.reps)
        bytes_of = {"jt": n * sz + 4 * (n + 1) + 8 * nnz + 2 * nnz * sz, "jv": m * sz + 4 * (m + 1) + 8 * nnz + 2 * nnz * sz}
        rec["products"] = {k: {"ms": t[0], "lowest_ms": t[1], "highest_ms": t[2], "bytes": bytes_of[k[:2]],
                               "tbps": round(bytes_of[k[:2]] / (t[0] * 1e9), 3),
                               "share_of_hbm_peak": round(bytes_of[k[:2]] / (t[0] * 1e9) / HBM_TBPS, 3)} for k, t in tm.items()}

        # ---- iterations and solves, 3 right-hand sides
        r3 = torch.from_numpy(rng.uniform(-1, 1, (m, 3))).cuda()
        with torch.no_grad():
            csq = CGLS.column_norms(pr, v)
            d = CGLS.damping_vector(pr, csq, DAMPING[0], DAMPING[1], v)
            jac = 1.0 / (csq + d)
        kinds = ["none", "jacobi"] + (["block_jacobi"] if int(np.max(sizes)) <= 32 else [])
        h, fns = {}, {}
        for steps in (10, 60):
            for k in kinds:
                fns["cgls_%s_%d" % (k, steps)] = (lambda k=k, steps=steps: S.lstsq_cg(
                    op, v, r3, damping=DAMPING, precond=None if k == "none" else k, tol=0.0, max_steps=steps))
            for k, pc in (("none", None), ("jacobi", jac)):
                fns["composed_%s_%d" % (k, steps)] = (lambda pc=pc, steps=steps: composed_cg(jpat, v, r3, d, pc, 0.0, steps))
        tm = timed_alternating(fns, a.warmup, a.reps)
        rec["fixed_steps_ms"] = {k: t for k, t in tm.items()}
        rec["per_iteration_ms"] = {k[:-3]: round((tm[k][0] - tm[k[:-3] + "_10"][0]) / 50.0, 5) for k in tm if k.endswith("_60")}
        rec["per_iteration_spread_ms"] = {k[:-3]: round(((tm[k][2] - tm[k][1]) + (tm[k[:-3] + "_10"][2] - tm[k[:-3] + "_10"][1])) / 50.0, 5)
                                          for k in tm if k.endswith("_60")}
        fns = {"lstsq": lambda: h.__setitem__("lstsq", S.lstsq(jpat, v, r3, damping=DAMPING))}
        for k in kinds:
            fns["cgls_" + k] = (lambda k=k: h.__setitem__("cgls_" + k, S.lstsq_cg(
                op, v, r3, damping=DAMPING, precond=None if k == "none" else k, tol=1e-10, max_steps=2000, return_info=True)))
        for k, pc in (("none", None), ("jacobi", jac)):
            fns["composed_" + k] = (lambda k=k, pc=pc: h.__setitem__("composed_" + k, composed_cg(jpat, v, r3, d, pc, 1e-10, 2000)))
        tm = timed_alternating(fns, a.warmup, a.reps)
        ref = h["lstsq"]
        sol = {"lstsq": {"ms": tm["lstsq"]}}
        for k in fns:
            if k == "lstsq":
                continue
            x, i = h[k]
            its = (i["iterations"] if isinstance(i, dict) else i.iterations()).tolist()
            stop = (i["stop"] if isinstance(i, dict) else i.stop()).tolist()
            sol[k] = {"ms": tm[k], "iterations": its, "stop": stop, "diff_to_lstsq": float((x - ref).norm() / ref.norm())}
        rec["to_tol_1e-10"] = sol
        emit(rec)
        del jpat, op, v, h, fns, ne, pr
        torch.cuda.empty_cache()

    # the BAL-871 stand-in from its counts: computed, not measured
    cams, pts, obs = 871, 527480, 2789783
    n871, m871 = 9 * cams + 3 * pts, 2 * obs + 9 * cams + 3 * pts
    nnz871 = 2 * obs * 12 + n871
    items871 = 2 * obs * (45 + 6) + n871
    emit({"problem": "bal871_computed", "m": m871, "order": n871, "nnz": nnz871,
          "row_bytes": 4 * (m871 + 1 + 2 * nnz871), "col_bytes": 4 * (n871 + 1 + 2 * nnz871 + cams * 9 + pts * 3),
          "plan_items": items871, "plan_bytes": 4 * (2 * (cams + pts + 1) + n871 + 3 * items871) + 8 * (cams + pts + 1),
          "note": "computed from the counts; every column is taken as long, an upper bound for the long list"})
    emit(dict(problem="ill_conditioned", **ill_conditioned(a)))


if __name__ == "__main__":
    main()
