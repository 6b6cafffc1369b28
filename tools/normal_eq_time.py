"""Time the normal equations of a sparse Jacobian (baspacho_amd.sparse) in fp64:
the hessian kernel, its adjoint and jt_vec alone, and sparse.lstsq forward and backward, with device
events, warmed up, median of --reps.  Beside them what the library offered before for the same problem:
the J^T J entries expanded in torch (one product per pair) and handed to section 14's assembly with
duplicates, then sparse.solve -- the same pairs, the same summation order, so the two layouts are
compared bit for bit before anything is timed.

Problems: a pose graph on GRID 82x82 (poses of 3 scalars; every edge of the grid structure gives 3
residual rows on its two poses, every pose a 3-row prior) and a small BAL-shaped problem (bench.py's
bal-small sizes: 120 cameras of 9, 40000 points of 3; every observation gives 2 rows on its camera and
its point, every param a prior row per scalar).

The rate of a kernel is its bytes over its event time against the 6.29 TB/s HBM peak of the MI355X.
hessian writes the layout and reads its part of the map and two gathered values per pair; the adjoint
writes the gradients of the values and reads its part of the map and two gathered values per term;
jt_vec writes g and reads the column lists, the values and one gathered value per entry.  One JSON line
per problem.

    python tools/normal_eq_time.py [--reps 5] [--warmup 2] [--only grid82,balsmall]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baspacho_amd import testing as T  # noqa: E402
from assemble_time import HBM_TBPS, timed  # noqa: E402


def _rows_on_params(groups, sizes, rows_per_group):
    """(rows, cols): every group of params gives rows_per_group residual rows, each on all the scalars
    of the group's params.  groups: int array [G, k] of param indices"""
    sizes = np.asarray(sizes, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    rows, cols, m = [], [], 0
    for shape in np.unique(sizes[groups], axis=0):
        sel = np.all(sizes[groups] == shape, axis=1)
        g = groups[sel]
        local = np.concatenate([np.arange(s) for s in shape])
        which = np.repeat(np.arange(len(shape)), shape)
        c = starts[g][:, which] + local[None, :]                        # [G, width]
        c = np.repeat(c, rows_per_group, axis=0)                        # [G * rpg, width]
        r = m + np.arange(len(c), dtype=np.int64)[:, None] + np.zeros_like(c)
        rows.append(r.ravel())
        cols.append(c.ravel())
        m += len(c)
    return np.concatenate(rows), np.concatenate(cols), m


def _jacobian(sizes, couples, rows_per_couple):
    """couples' rows, then one prior row per scalar"""
    r1, c1, m1 = _rows_on_params(couples, sizes, rows_per_couple)
    n = int(np.sum(sizes))
    rows = np.concatenate([r1, m1 + np.arange(n)])
    cols = np.concatenate([c1, np.arange(n)])
    rng = np.random.default_rng(37)
    vals = np.concatenate([rng.uniform(-1.0, 1.0, len(r1)), np.full(n, 2.0)])
    return rows, cols, vals, m1 + n, n


def problems():
    def grid82():
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
        sizes = np.full(ss.order(), 3, dtype=np.int64)
        br = np.repeat(np.arange(ss.order()), np.diff(ss.ptrs))
        bc = np.asarray(ss.inds, dtype=np.int64)
        off = br != bc
        return sizes, _jacobian(sizes, np.stack([br[off], bc[off]], axis=1), 3)

    def balsmall():
        sizes, _, cam, pt = T.gen_bal_synthetic(num_cams=120, num_pts=40000, band=16)
        cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
        if cam.max() < 120:  # camera params follow the points
            cam = cam + 40000
        return np.asarray(sizes, dtype=np.int64), _jacobian(sizes, np.stack([cam, pt], axis=1), 2)

    return {"grid82": grid82, "balsmall": balsmall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,balsmall")
    a = ap.parse_args()
    import torch
    from baspacho_amd import sparse as S
    for name in a.only.split(","):
        sizes, (rows, cols, vals, m, n) = problems()[name]()
        t0 = time.perf_counter()
        jpat = S.JacobianPattern(rows, cols, m, n, param_sizes=sizes)
        t_map = time.perf_counter() - t0
        sol, ne = jpat.solver, jpat.normal_eq
        info = ne.info()
        nnz, ds, P, terms, sz = len(rows), sol.dataSize(), info["pairs"], info["adjoint_terms"], 8
        v = torch.from_numpy(vals).cuda()
        r = torch.randn(m, dtype=torch.float64, device="cuda")
        data = ne.hessian(v)
        gv, g = torch.empty_like(v), torch.empty(n, dtype=torch.float64, device="cuda")
        rec = {"problem": name, "m": m, "order": n, "nnz": nnz, "data_size": ds, "pairs": P,
               "destinations": info["destinations"], "max_run": info["max_run"], "long_runs": info["long_runs"],
               "map_build_s": round(t_map, 2), "forward_bytes": info["forward_bytes"],
               "adjoint_bytes": info["adjoint_bytes"], "vector_bytes": info["vector_bytes"], "hbm_peak_tbps": HBM_TBPS}
        t = timed(lambda: ne.hessian(v, out=data), a.warmup, a.reps)
        rec["hessian_ms"], rec["hessian_tbps"] = t, round((ds * sz + info["forward_bytes"] + 2 * P * sz) / (t * 1e9), 3)
        t = timed(lambda: ne.hessianAdjoint(v, data, out=gv), a.warmup, a.reps)
        rec["adjoint_ms"], rec["adjoint_tbps"] = t, round((nnz * sz + info["adjoint_bytes"] + 2 * terms * sz) / (t * 1e9), 3)
        t = timed(lambda: ne.jtVec(v, r, out=g), a.warmup, a.reps)
        rec["jt_vec_ms"], rec["jt_vec_tbps"] = t, round((n * sz + 4 * (n + 1) + 8 * nnz + 2 * nnz * sz) / (t * 1e9), 3)

        # the same problem through expand-then-assemble: one entry of J^T J per pair, in run order
        ka, kb, _ = ne.pairTable()
        pat = S.SymmetricPattern(cols[ka], cols[kb], n, param_sizes=sizes)
        assert pat.solver.dataSize() == ds
        ia, ib = torch.from_numpy(ka.astype(np.int64)).cuda(), torch.from_numpy(kb.astype(np.int64)).cuda()
        expand = lambda vv: vv.index_select(0, ia) * vv.index_select(0, ib)
        rec["equal_bits"] = bool(torch.equal(pat.assembly.assemble(expand(v)), data))
        out2 = torch.empty_like(data)
        rec["expand_assemble_ms"] = timed(lambda: pat.assembly.assemble(expand(v), out=out2), a.warmup, a.reps)
        for fname in ("lstsq", "expand_solve"):
            vv = v.clone().requires_grad_(True)
            rr = r.clone().requires_grad_(True)
            holder = {}

            def fwd():
                if fname == "lstsq":
                    holder["loss"] = S.lstsq(jpat, vv, rr).sum()
                else:
                    holder["loss"] = S.solve(pat, expand(vv), S.jt_vec(jpat, vv, rr)).sum()

            def bwd():
                holder["loss"].backward(retain_graph=True)
            rec[fname + "_fwd_ms"] = timed(fwd, a.warmup, a.reps)
            rec[fname + "_bwd_ms"] = timed(bwd, a.warmup, a.reps)
            del holder
        print(json.dumps(rec), flush=True)
        del jpat, pat, sol, ne, data, out2, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
