"""Time the device-resident Lanczos recurrence of DESIGN.md section 25 in fp64, with device events, warmed up,
median of --reps; the routes of one comparison are timed in one run, alternating (tools/sym_product_time.py's
timer).

  sparse.lanczos at 32 steps for reorth None and "full", with 1 and 16 start vectors (check_every None: nothing
      read), beside a plain torch loop of the same recurrence on the same operator (SymProduct.mv): torch dot
      products, the reorthogonalisation as two dense products with the basis (c = V w, w -= V^T c, twice), and
      one host read of beta per step, which is what decides a breakdown in a caller-side loop.  Reported: the
      total and total / 32, the average step (with "full" a step's cost grows with the step number).
  the project and the subtract pieces alone at step 31 (32 basis vectors), and the bytes per second they
      reach: project reads 33 n q values, subtract reads 33 and writes 1.
  logdet_slq (16 probes, 32 steps) beside S.logdet, and the estimate's error against it.

Problems as in tools/cg_time.py: GRID 82x82 and the BAL-871 stand-in with the same diagonally dominant values.
One JSON line per problem, printed and written to profiles/lanczos_time.txt (--out).  launches_per_step is
counted from the launch sequence of section 25, not traced.

    python tools/lanczos_time.py [--reps 5] [--warmup 2] [--only grid82,bal871] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from assemble_time import block_entries, problems  # noqa: E402
from sym_product_time import timed_alternating  # noqa: E402

STEPS = 32
LAUNCHES = {"none": 6, "full": 12}


def torch_loop(prod, v, v0, steps, full):
    """the same recurrence with torch operations: (alpha, beta) lists of [q] tensors; one host read per step"""
    import torch
    n, q = v0.shape
    V = torch.zeros((steps, n, q), dtype=v0.dtype, device=v0.device)
    V[0] = v0 / v0.norm(dim=0)
    alphas, betas = [], []
    beta = None
    for j in range(steps):
        w = prod.mv(v, V[j])
        alpha = (V[j] * w).sum(0)
        w -= alpha * V[j]
        if j > 0:
            w -= beta * V[j - 1]
        if full:
            Vj = V[:j + 1]
            for _ in range(2):
                if q == 1:
                    w -= (Vj[:, :, 0].T @ (Vj[:, :, 0] @ w[:, 0])).unsqueeze(-1)
                else:
                    w -= torch.einsum("knq,kq->nq", Vj, torch.einsum("knq,nq->kq", Vj, w))
        beta = w.norm(dim=0)
        alphas.append(alpha)
        betas.append(beta)
        if float(beta.min()) == 0.0:  # the host read: a breakdown ends the loop
            break
        if j + 1 < steps:
            V[j + 1] = w / beta
    return alphas, betas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,bal871")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lanczos_time.txt"),
                    help="the JSON lines go to this file as well (overwritten)")
    a = ap.parse_args()
    open(a.out, "w").close()
    import torch
    from baspacho_amd import lanczos as lz
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
        rec = {"problem": name, "order": n, "nnz": nnz, "steps": STEPS, "reps": a.reps, "warmup": a.warmup,
               "launches_per_step": LAUNCHES}

        # ---- the recurrence beside the torch loop
        h = {}
        for q in (1, 16):
            v0 = torch.from_numpy(lz.rademacher(n, q, 3)).cuda()
            fns = {}
            for reorth in (None, "full"):
                tag = "%s_q%d" % (reorth or "none", q)
                fns["device_" + tag] = (lambda reorth=reorth, tag=tag, v0=v0: h.__setitem__(
                    tag, S.lanczos(pat, v, v0, steps=STEPS, reorth=reorth, check_every=None)))
                fns["loop_" + tag] = (lambda reorth=reorth, tag=tag, v0=v0: h.__setitem__(
                    "loop_" + tag, torch_loop(prod, v, v0, STEPS, reorth == "full")))
            tm = timed_alternating(fns, a.warmup, a.reps)
            print("%s: q = %d timed" % (name, q), file=sys.stderr, flush=True)
            for k, t in tm.items():
                rec[k + "_ms"] = t
                rec[k + "_per_step_ms"] = round(t / STEPS, 5)
            for reorth in ("none", "full"):
                tag = "%s_q%d" % (reorth, q)
                al = torch.stack(h["loop_" + tag][0], dim=-1)
                rec["alpha_diff_to_loop_" + tag] = float((h[tag]["alpha"].reshape(al.shape) - al).abs().max() / al.abs().max())
            h.clear()

            # ---- project and subtract alone at step 31
            run = lz.LanczosRun(sol, v0, S._entries_operator(pat, v, q), STEPS)
            run.start()
            for _ in range(STEPS - 1):
                run.iterate()
            assert run.running()
            cnt = ctypes.c_int64(STEPS)
            fns = {"project_q%d" % q: lambda run=run: run._piece("project", run._w, cnt),
                   "subtract_q%d" % q: lambda run=run: run._piece("subtract", run._w, cnt, ctypes.c_int32(0), run._coef)}
            tm = timed_alternating(fns, a.warmup, a.reps)
            for k, t in tm.items():
                moved = (STEPS + (1 if k.startswith("project") else 2)) * n * q * 8
                rec[k + "_ms"] = t
                rec[k + "_TB_per_s"] = round(moved / (t * 1e-3) / 1e12, 4)
            del run, v0
            torch.cuda.empty_cache()

        # ---- logdet_slq beside the factor
        fns = {"logdet": lambda: h.__setitem__("ld", S.logdet(pat, v)),
               "logdet_slq": lambda: h.__setitem__("slq", S.logdet_slq(pat, v, probes=16, steps=STEPS, return_info=True))}
        tm = timed_alternating(fns, a.warmup, a.reps)
        rec.update({k + "_ms": t for k, t in tm.items()})
        ld, (est, info) = float(h["ld"]), h["slq"]
        rec.update({"logdet": ld, "logdet_slq": float(est), "logdet_slq_stderr": float(info["stderr"]),
                    "logdet_slq_rel_error": abs(float(est) - ld) / abs(ld)})
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del pat, prod, sol, v, h, fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
