"""Time f(A) v from the Lanczos basis in fp64, with device events, warmed up, median of
--reps; the routes of one comparison are timed in one run, alternating (tools/sym_product_time.py's timer).

  the combine over 32 slots (bsp_krylov_combine_*, 1 and 2 outputs) beside the subtract piece of the
      reorthogonalisation over the same 32 slots (lzSubtract: the same bytes read, one vector written, plus its
      partial sums) and torch.einsum over the [32, n, q] basis, with 1 and 16 columns, and the bytes per second
      they reach: combine moves (32 + nf) n q values, subtract 34 n q, einsum 33 n q.
  sample_lanczos at 32 steps of the plain recurrence, with the basis kept and with the two-pass route, beside
      S.sample (assemble, factor, one triangular solve), and the indicator `change` the 32 steps end with.

Problems as in tools/lanczos_time.py: GRID 82x82 and the BAL-871 stand-in with the same diagonally dominant
values.  One JSON line per problem, printed and written to profiles/matfun_time.txt (--out).

    python tools/matfun_time.py [--reps 5] [--warmup 2] [--only grid82,bal871] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,bal871")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matfun_time.txt"),
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
        sol = pat.solver
        rng = np.random.default_rng(37)
        vals = rng.uniform(-1.0, 1.0, nnz)
        off = rows != cols
        rowsum = np.zeros(n)
        np.add.at(rowsum, rows[off], np.abs(vals[off]))
        np.add.at(rowsum, cols[off], np.abs(vals[off]))
        vals[~off] = 1.05 * rowsum[rows[~off]] + 0.1
        v = torch.from_numpy(vals).cuda()
        rec = {"problem": name, "order": n, "nnz": nnz, "steps": STEPS, "reps": a.reps, "warmup": a.warmup}
        h = {}
        for q in (1, 16):
            v0 = torch.from_numpy(lz.rademacher(n, q, 3)).cuda()

            # ---- combine, subtract and einsum over the 32 slots of one basis
            run = lz.LanczosRun(sol, v0, S._entries_operator(pat, v, q), STEPS)
            run.start()
            for _ in range(STEPS - 1):
                run.iterate()
            assert run.running()
            cnt = ctypes.c_int64(STEPS)
            limit = torch.full((q,), STEPS, dtype=torch.int64, device="cuda")
            ys = {nf: torch.from_numpy(rng.uniform(-1, 1, (q, nf, STEPS))).cuda() for nf in (1, 2)}
            outs = {nf: torch.empty((nf, n, q), dtype=torch.float64, device="cuda") for nf in (1, 2)}
            yk = ys[1][:, 0, :].t().contiguous()   # [k, q]
            fns = {"subtract_q%d" % q: lambda run=run: run._piece("subtract", run._w, cnt, ctypes.c_int32(0), run._coef),
                   "combine_nf1_q%d" % q: lambda run=run: run.combine(ys[1], limit, outs[1], count=STEPS),
                   "combine_nf2_q%d" % q: lambda run=run: run.combine(ys[2], limit, outs[2], count=STEPS),
                   "einsum_q%d" % q: lambda run=run: h.__setitem__("e", torch.einsum("knq,kq->nq", run.basis, yk))}
            tm = timed_alternating(fns, a.warmup, a.reps)
            moved = {"subtract": STEPS + 2, "combine_nf1": STEPS + 1, "combine_nf2": STEPS + 2, "einsum": STEPS + 1}
            for k, t in tm.items():
                rec[k + "_ms"] = t
                rec[k + "_TB_per_s"] = round(moved[k[:k.rindex("_q")]] * n * q * 8 / (t * 1e-3) / 1e12, 4)
            rec["combine_diff_to_einsum_q%d" % q] = float((outs[1][0] - h["e"]).abs().max() / h["e"].abs().max())
            del run, ys, outs, yk, fns
            h.clear()
            torch.cuda.empty_cache()
            print("%s: q = %d kernels timed" % (name, q), file=sys.stderr, flush=True)

            # ---- sample_lanczos beside the factor's sample
            z = torch.from_numpy(rng.standard_normal((n, q))).cuda()
            kw = dict(steps=STEPS, reorth=None, return_info=True)
            fns = {"sample_q%d" % q: lambda z=z: h.__setitem__("s", S.sample(pat, v, z)),
                   "sample_lanczos_basis_q%d" % q: lambda z=z: h.__setitem__("b", S.sample_lanczos(pat, v, z, **kw)),
                   "sample_lanczos_two_pass_q%d" % q: lambda z=z: h.__setitem__(
                       "t", S.sample_lanczos(pat, v, z, memory="two_pass", **kw))}
            tm = timed_alternating(fns, a.warmup, a.reps)
            rec.update({k + "_ms": t for k, t in tm.items()})
            rec["two_pass_bitwise_basis_q%d" % q] = bool(torch.equal(h["b"][0], h["t"][0]))
            rec["change_max_q%d" % q] = float(h["b"][1]["change"].max())
            # both routes sample N(0, A^-1), by different maps: |x|_A^2 = |z|^2 for either
            for tag, x in (("sample", h["s"]), ("sample_lanczos", h["b"][0])):
                qa = (x * S.matvec(pat, v, x)).sum(0)
                rec["%s_xAx_over_zz_q%d" % (tag, q)] = [round(float(r), 12) for r in (qa / (z * z).sum(0))[:2]]
            del z, fns, v0
            h.clear()
            torch.cuda.empty_cache()
            print("%s: q = %d samples timed" % (name, q), file=sys.stderr, flush=True)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del pat, sol, v, h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
