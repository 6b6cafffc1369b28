"""Time the implicit Schur elimination of DESIGN.md section 29 in fp64, with device events, warmed up, median of
--reps with the lowest and highest repetition beside it; the routes of one comparison are timed in one process,
alternating (tools/cgls_time.py's protocol).  The problem is tools/normal_eq_time.py's small BAL shape with its
40 000 points eliminated.

  The host build time and the device bytes of the map and of both block plans (eliminated and kept params).
  The product S p (q = 1) of the map (two launches) against the composed route of existing entries: p scattered
      into a zero full-length vector, jVec, jtVec, the eliminated blocks applied by a torch batched product, jVec
      of the zero-padded y, the subtraction, jtVec, the gather of the kept part and the damping.
  One iteration with 3 right-hand sides = (t60 - t10) / 50 at tol = 0, and the solve to tol = 1e-10, for none /
      jacobi / block_jacobi, with and without eliminate, with sparse.lstsq (the factor) beside them and the
      difference to it.
  The sizes for the BAL-871 stand-in computed from its counts (not measured).

One JSON line per record, printed and written to profiles/schur_time.txt (--out).

    python tools/schur_time.py [--reps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cgls_time import DAMPING, timed_alternating  # noqa: E402
from normal_eq_time import problems  # noqa: E402

NUM_PTS = 40000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_time.txt"),
                    help="the JSON lines go to this file as well (overwritten)")
    a = ap.parse_args()
    open(a.out, "w").close()
    import torch
    from baspacho_amd import cgls as CGLS
    from baspacho_amd import sparse as S
    emit = lambda rec: (print(json.dumps(rec), flush=True), open(a.out, "a").write(json.dumps(rec) + "\n"))
    sizes, (rows, cols, vals, m, n) = problems()["balsmall"]()
    assert (sizes[:NUM_PTS] == 3).all()
    elim = np.arange(NUM_PTS, dtype=np.int64)
    op = S.JacobianOperator(rows, cols, m, n, param_sizes=sizes)
    t0 = time.perf_counter()
    sch = S.JacobianSchur(op, elim)
    t_map = time.perf_counter() - t0
    t0 = time.perf_counter()
    kept_plan = sch.map.precondInfo("block_jacobi")
    t_kept = time.perf_counter() - t0
    t0 = time.perf_counter()
    full_plan = op.product.precondInfo("block_jacobi")
    t_full = time.perf_counter() - t0
    si = sch.info()
    rec = {"problem": "balsmall", "m": m, "order": n, "nnz": len(rows), "eliminated_params": NUM_PTS, "n_kept": sch.nK,
           "n_elim": sch.nE, "reps": a.reps, "warmup": a.warmup, "damping": DAMPING,
           "map": {"host_build_s": round(t_map, 3), "map_bytes": si["map_bytes"], "elim_plan_bytes": si["plan_bytes"],
                   "elim_plan_items": si["block_items"], "max_group": si["max_group"], "free_rows": si["free_rows"],
                   "long_cols_kept": si["long_cols_kept"]},
           "kept_plan": {"host_build_s": round(t_kept, 3), "bytes": kept_plan["device_bytes"], "items": kept_plan["items"]},
           "full_plan": {"host_build_s": round(t_full, 3), "bytes": full_plan["device_bytes"], "items": full_plan["items"]}}
    v = torch.from_numpy(vals).cuda()
    rng = np.random.default_rng(37)
    pr, smap = op.product, sch.map
    kept = sch.kept_scalars(v.device)
    es = torch.from_numpy(smap.table()["elim_scalar"].astype(np.int64)).cuda()
    with torch.no_grad():
        csq = CGLS.column_norms(pr, v)
        d = CGLS.damping_vector(pr, csq, DAMPING[0], DAMPING[1], v)
        binv, status = smap.build(v, d)
    assert status.tolist() == [-1, 0]
    p = torch.from_numpy(rng.uniform(-1, 1, sch.nK)).cuda()
    out, t = torch.empty_like(p), torch.empty(m, 1, dtype=v.dtype, device=v.device)
    blocks = binv[:9 * NUM_PTS].reshape(NUM_PTS, 3, 3)
    dk = d[kept]

    def composed():
        pf = torch.zeros(n, dtype=v.dtype, device=v.device)
        pf[kept] = p
        av = pr.jVec(v, pf)
        u = pr.jtVec(v, av)
        yf = torch.zeros_like(pf)
        yf[es] = torch.bmm(blocks, u[es].reshape(NUM_PTS, 3, 1)).reshape(-1)
        tv = av - pr.jVec(v, yf)
        return pr.jtVec(v, tv)[kept] + dk * p

    fused = lambda: smap.mv(v, binv, p, d=d, out=out, t=t)
    ref = composed()
    rec["product_diff_to_composed"] = float((fused() - ref).norm() / ref.norm())
    tm = timed_alternating({"schur_mv": fused, "composed": composed}, a.warmup, a.reps)
    rec["product_ms"] = tm
    spread = sum(tm[k][2] - tm[k][1] for k in tm)
    rec["product_condition"] = {"schur_minus_composed_ms": round(tm["schur_mv"][0] - tm["composed"][0], 4),
                                "summed_spreads_ms": round(spread, 4),
                                "holds": bool(tm["schur_mv"][0] - tm["composed"][0] <= spread)}

    # ---- iterations and solves, 3 right-hand sides
    r3 = torch.from_numpy(rng.uniform(-1, 1, (m, 3))).cuda()
    kinds = ["none", "jacobi", "block_jacobi"]
    routes = {"plain": None, "schur": sch}
    fns = {}
    for steps in (10, 60):
        for k in kinds:
            for rn, el in routes.items():
                fns["%s_%s_%d" % (rn, k, steps)] = (lambda k=k, el=el, steps=steps: S.lstsq_cg(
                    op, v, r3, damping=DAMPING, precond=None if k == "none" else k, tol=0.0, max_steps=steps, eliminate=el))
    tm = timed_alternating(fns, a.warmup, a.reps)
    rec["fixed_steps_ms"] = tm
    rec["per_iteration_ms"] = {k[:-3]: round((tm[k][0] - tm[k[:-3] + "_10"][0]) / 50.0, 5) for k in tm if k.endswith("_60")}
    jpat = S.JacobianPattern(rows, cols, m, n, param_sizes=sizes)
    h = {}
    fns = {"lstsq": lambda: h.__setitem__("lstsq", S.lstsq(jpat, v, r3, damping=DAMPING))}
    for k in kinds:
        for rn, el in routes.items():
            fns["%s_%s" % (rn, k)] = (lambda k=k, el=el, rn=rn: h.__setitem__("%s_%s" % (rn, k), S.lstsq_cg(
                op, v, r3, damping=DAMPING, precond=None if k == "none" else k, tol=1e-10, max_steps=2000, return_info=True,
                eliminate=el)))
    tm = timed_alternating(fns, a.warmup, a.reps)
    xl = h["lstsq"]
    sol = {"lstsq": {"ms": tm["lstsq"]}}
    for k in fns:
        if k != "lstsq":
            x, i = h[k]
            sol[k] = {"ms": tm[k], "iterations": i["iterations"].tolist(), "stop": i["stop"].tolist(),
                      "diff_to_lstsq": float((x - xl).norm() / xl.norm())}
    rec["to_tol_1e-10"] = sol
    emit(rec)

    # the BAL-871 stand-in from its counts: computed, not measured
    cams, pts, obs = 871, 527480, 2789783
    n871, m871 = 9 * cams + 3 * pts, 2 * obs + 9 * cams + 3 * pts
    kept_e, elim_e = 2 * obs * 9 + 9 * cams, 2 * obs * 3 + 3 * pts
    lists = 4 * (2 * (m871 + 1) + (3 * pts + 1) + (9 * cams + 1) + 4 * (kept_e + elim_e) + 9 * cams)
    other = 4 * ((pts + 1) + 9 * cams + 3 * pts + (pts + 1) + m871)
    elim_items, kept_items = 2 * obs * 6 + 3 * pts, 2 * obs * 45 + 9 * cams
    emit({"problem": "bal871_computed", "m": m871, "order": n871, "n_kept": 9 * cams, "n_elim": 3 * pts,
          "map_bytes": lists + other, "elim_plan_items": elim_items,
          "elim_plan_bytes": 4 * (2 * (pts + 1) + pts + n871 + 3 * elim_items) + 8 * (pts + 1),
          "kept_plan_items": kept_items, "kept_plan_bytes": 4 * (2 * (cams + 1) + cams + n871 + 3 * kept_items) + 8 * (cams + 1),
          "cg_vectors_bytes_q1": 8 * 9 * cams * 5, "t_bytes_q1": 8 * m871,
          "note": "computed from the counts; every kept column is taken as long, an upper bound for the long list"})


if __name__ == "__main__":
    main()
