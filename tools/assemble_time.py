"""Time the coordinate-entry assembly (baspacho_amd.sparse): the assemble and
adjoint kernels alone, and sparse.solve forward and backward next to autograd.solve on pre-assembled
data, with device events, warmed up, median of --reps.  Problems as in tools/autograd_time.py: BAL-871
(synthetic), GRID 82x82 and MERI.  Entries: every element of every block of the input structure (the
lower one of a diagonal block), without fill; the `dup` variant splits each entry into 1..8
contributions in shuffled order.  The rate of a kernel is its bytes over its event time, against the
6.29 TB/s HBM peak of the MI355X: assemble writes the layout and reads the values and the map (run
entries, run starts, element positions, tile index); the adjoint writes the gradients of the values
and reads the entry offsets and one gathered element per entry.  One JSON line per problem and variant.

    python tools/assemble_time.py [--reps 5] [--warmup 2] [--only bal871,grid82,meri]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baspacho_amd import testing as T  # noqa: E402

HBM_TBPS = 6.29


def problems():
    def bal871():
        sizes, ss, _, _ = T.gen_bal_synthetic()
        return sizes, ss

    def grid82():
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
        return np.full(ss.order(), 3, dtype=np.int64), ss

    def meri():
        ss = T.gen_meridians(4, 1500, 0.5, 120, 600, 2, 2, 37)
        return np.full(ss.order(), 3, dtype=np.int64), ss

    return {"bal871": bal871, "grid82": grid82, "meri": meri}


def block_entries(sizes, ss):
    """(rows, cols) of every element of every lower block of the structure, diagonal blocks lower only"""
    sizes = np.asarray(sizes, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    br = np.repeat(np.arange(len(sizes)), np.diff(ss.ptrs))
    bc = np.asarray(ss.inds, dtype=np.int64)
    rows, cols = [], []
    for sp in np.unique(sizes):
        for sq in np.unique(sizes):
            for diag in (False, True):
                sel = (sizes[br] == sp) & (sizes[bc] == sq) & ((br == bc) == diag)
                if not sel.any():
                    continue
                ro, co = np.meshgrid(np.arange(sp), np.arange(sq), indexing="ij")
                ro, co = ro.ravel(), co.ravel()
                if diag:
                    ro, co = ro[ro >= co], co[ro >= co]
                rows.append((starts[br[sel]][:, None] + ro[None, :]).ravel())
                cols.append((starts[bc[sel]][:, None] + co[None, :]).ravel())
    return np.concatenate(rows), np.concatenate(cols)


def timed(fn, warmup, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82,meri")
    a = ap.parse_args()
    import torch
    from baspacho_amd import autograd as BA
    from baspacho_amd import sparse as S
    for name in a.only.split(","):
        sizes, ss = problems()[name]()
        r0, c0 = block_entries(sizes, ss)
        # BAL-871 has 78.5 M entries without duplicates; split 1..8 ways they would need ~350 M (GBs of host
        # memory for the map): the duplicated variant runs on GRID and MERI only
        for variant in (["plain"] if name == "bal871" else ["plain", "dup"]):
            rng = np.random.default_rng(37)
            rows, cols = r0, c0
            if variant == "dup":
                reps = rng.integers(1, 9, size=len(r0))
                order = rng.permutation(int(reps.sum()))
                rows, cols = np.repeat(r0, reps)[order], np.repeat(c0, reps)[order]
            n = int(np.sum(sizes))
            t0 = time.perf_counter()
            pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes)
            t_map = time.perf_counter() - t0
            sol, asm = pat.solver, pat.assembly
            info = asm.info()
            runs = np.bincount(np.searchsorted(np.unique(asm.entryOffsets()), asm.entryOffsets()))
            vals = rng.uniform(-1.0, 1.0, len(rows))
            vals[rows == cols] = n * 1.2  # diagonally dominant: the factor exists
            v = torch.from_numpy(vals).cuda()
            ds, nnz, sz = sol.dataSize(), len(rows), 8
            data = asm.assemble(v)
            gv = torch.empty_like(v)
            t_asm = timed(lambda: asm.assemble(v, out=data), a.warmup, a.reps)
            t_adj = timed(lambda: asm.adjoint(data, out=gv), a.warmup, a.reps)
            map_fwd = info["device_bytes"] - 8 * nnz  # the forward does not read the entry offsets
            asm_bytes = ds * sz + info["kept"] * sz + map_fwd
            adj_bytes = nnz * sz + 8 * nnz + info["kept"] * sz
            rec = {"problem": name, "variant": variant, "order": n, "data_size": ds, "nnz": nnz,
                   "elements": info["elements"], "median_run": float(np.median(runs)), "max_run": info["max_run"],
                   "map_build_s": round(t_map, 2), "map_device_bytes": info["device_bytes"],
                   "assemble_ms": t_asm, "assemble_tbps": round(asm_bytes / (t_asm * 1e9), 3),
                   "adjoint_ms": t_adj, "adjoint_tbps": round(adj_bytes / (t_adj * 1e9), 3),
                   "hbm_peak_tbps": HBM_TBPS}
            rec["clone_ms"] = timed(lambda: data.clone(), a.warmup, a.reps)
            b = torch.randn(n, dtype=torch.float64, device="cuda")
            bi = pat.toInternal(b)
            for fname in ("sparse_solve", "autograd_solve"):
                vv = v.clone().requires_grad_(True)
                dd = data.clone().requires_grad_(True)
                bb = (b if fname == "sparse_solve" else bi).clone().requires_grad_(True)
                holder = {}

                def fwd():
                    if fname == "sparse_solve":
                        holder["loss"] = S.solve(pat, vv, bb).sum()
                    else:
                        holder["loss"] = BA.solve(sol, dd, bb).sum()

                def bwd():
                    holder["loss"].backward(retain_graph=True)
                rec[fname + "_fwd_ms"] = timed(fwd, a.warmup, a.reps)
                rec[fname + "_bwd_ms"] = timed(bwd, a.warmup, a.reps)
                del holder
            print(json.dumps(rec), flush=True)
            del pat, sol, asm, data, gv, v
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
