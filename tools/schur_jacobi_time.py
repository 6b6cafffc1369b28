"""Time the block diagonal of S as preconditioner of the implicit Schur iteration in fp64, by
tools/schur_time.py's protocol: device events, warmed up, median of --reps with the lowest and highest repetition
beside it, the routes of one comparison timed in one process, alternating; the small BAL shape with its 40 000
points eliminated.

  The host build time and the device bytes of the new plan beside those of the kept item plan of "block_jacobi".
  The build: schurJacobiBuild (both launches and the status) against the "block_jacobi" build of the kept blocks
      (bsp_jac_schur_precond_build_* kind 2).  With --parent-lib PATH that build is taken from the library at PATH
      (the parent commit's), loaded beside this one into the same process on a map of its own.
  The solve to tol = 1e-10 with 3 right-hand sides for none / jacobi / block_jacobi / schur_jacobi with eliminate,
      sparse.lstsq (the factor) beside them and the difference to it.
  The plan's size for the BAL-871 stand-in computed from its counts (not measured).

One JSON line per record, printed and written to profiles/schur_jacobi_time.txt (--out).

    python tools/schur_jacobi_time.py [--reps 5] [--warmup 2] [--parent-lib PATH] [--out FILE]
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


class bound_to:
    """objects built inside bind to the library at `path` instead of the package's own"""

    def __init__(self, path):
        from baspacho_amd import _lib as L
        self.L = L
        own, own_path = L._lib, L.LIB_PATH
        L._lib, L.LIB_PATH = None, path
        try:
            self.other = L.load()
        finally:
            L._lib, L.LIB_PATH = own, own_path

    def __enter__(self):
        self.own, self.L._lib = self.L._lib, self.other

    def __exit__(self, *exc):
        self.L._lib = self.own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="the library whose kind-2 build is the comparison's other route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_jacobi_time.txt"),
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
    sch = S.JacobianSchur(op, elim)
    smap, pr = sch.map, op.product
    t0 = time.perf_counter()
    plan = smap.schurJacobiInfo()
    t_plan = time.perf_counter() - t0
    assert not plan["kept_item_plan_built"]
    if a.parent_lib:
        with bound_to(a.parent_lib):
            op2 = S.JacobianOperator(rows, cols, m, n, param_sizes=sizes)
            sch2 = S.JacobianSchur(op2, elim)
    else:
        op2, sch2 = op, sch
    t0 = time.perf_counter()
    kept_plan = sch2.map.precondInfo("block_jacobi")
    t_kept = time.perf_counter() - t0
    rec = {"problem": "balsmall", "m": m, "order": n, "nnz": len(rows), "eliminated_params": NUM_PTS, "n_kept": sch.nK,
           "reps": a.reps, "warmup": a.warmup, "damping": DAMPING,
           "block_jacobi_build_from": "the library given as --parent-lib" if a.parent_lib else "this library",
           "schur_jacobi_plan": dict(plan, host_build_s=round(t_plan, 3)),
           "kept_item_plan": {"host_build_s": round(t_kept, 3), "bytes": kept_plan["device_bytes"],
                              "items": kept_plan["items"]}}
    v = torch.from_numpy(vals).cuda()
    rng = np.random.default_rng(37)
    with torch.no_grad():
        csq = CGLS.column_norms(pr, v)
        d = CGLS.damping_vector(pr, csq, DAMPING[0], DAMPING[1], v)
        binv, status = smap.build(v, d)
        assert status.tolist() == [-1, 0]
        partials = torch.empty(max(plan["partial_elems"], 1), dtype=torch.float64, device="cuda")
        minv = torch.empty(plan["inverse_elems"], dtype=v.dtype, device="cuda")
        fns = {"schur_jacobi_build": lambda: smap.schurJacobiBuild(v, binv, d, partials=partials, out=minv),
               "block_jacobi_build": lambda: sch2.map.precondBuild("block_jacobi", v, None, d)}
        s_status = fns["schur_jacobi_build"]()[1].tolist()
        c_minv, c_status = fns["block_jacobi_build"]()
        assert s_status == [-1, 0] and c_status.tolist() == [-1, 0]
        # (the blocks of S against those of C: the same offsets, the difference is F^T B^-1 F)
        rec["blocks_rel_diff_S_to_C"] = float((minv - c_minv).norm() / c_minv.norm())
        tm = timed_alternating(fns, a.warmup, a.reps)
    rec["build_ms"] = tm
    spread = sum(tm[k][2] - tm[k][1] for k in tm)
    diff = tm["schur_jacobi_build"][0] - tm["block_jacobi_build"][0]
    rec["build_condition"] = {"schur_jacobi_minus_block_jacobi_ms": round(diff, 4), "summed_spreads_ms": round(spread, 4),
                              "holds": bool(-diff > spread)}

    # ---- the solve to tol = 1e-10, 3 right-hand sides
    r3 = torch.from_numpy(rng.uniform(-1, 1, (m, 3))).cuda()
    jpat = S.JacobianPattern(rows, cols, m, n, param_sizes=sizes)
    h = {}
    fns = {"lstsq": lambda: h.__setitem__("lstsq", S.lstsq(jpat, v, r3, damping=DAMPING))}
    for k in ("none", "jacobi", "block_jacobi", "schur_jacobi"):
        fns["schur_" + k] = (lambda k=k: h.__setitem__("schur_" + k, S.lstsq_cg(
            op, v, r3, damping=DAMPING, precond=None if k == "none" else k, tol=1e-10, max_steps=2000, return_info=True,
            eliminate=sch)))
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

    # the BAL-871 stand-in from its counts: computed, not measured.  A pair is an observation
    # (2 rows, 9 + 3 record entries each); the 9 rows of no group of a camera are one pseudo-pair
    cams, obs = 871, 2789783
    pairs, pair_rows, record = obs + cams, 2 * obs + 9 * cams, 2 * obs * 12 + 9 * cams * 9
    chunks = obs // 64 + 2 * cams  # (an upper bound: every camera's last chunk is partial)
    emit({"problem": "bal871_computed", "pairs": pairs, "pair_rows": pair_rows, "record_entries": record,
          "chunks_at_most": chunks, "partial_bytes_at_most": 8 * 45 * chunks,
          "plan_bytes": 4 * (record + 3 * pairs + 2 * chunks + 2 * cams) + 8 * (chunks + cams),
          "kept_item_plan_bytes": 4 * (2 * (cams + 1) + cams + (9 * cams + 3 * 527480) + 3 * (2 * obs * 45 + 9 * cams))
          + 8 * (cams + 1),
          "note": "computed from the counts, not measured"})


if __name__ == "__main__":
    main()
