"""Time Solver.inverseBlocks (reach solves) for random param pairs against the two
routes that exist without it, in one session: unit columns written with torch + the full solve() with the
same number of right-hand sides + a gather (in the same chunks of at most 512 columns), and one
selectedInverse() (which holds a pair only if it is on the pattern of L).  fp64, wall clock between device
synchronisations (the host work of a call -- the plan of its queries -- is part of what a caller waits
for), median of --reps after --warmup; the data is damped as tools/selinv_time.py does.  One JSON line per
problem, kind of pair and number of pairs.

    python tools/inverse_blocks_time.py [--reps 5] [--warmup 2] [--only grid82,bal871] [--pairs 16,128,1024]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import baspacho_amd as B  # noqa: E402
from baspacho_amd import testing as T  # noqa: E402

NUM_PTS, NUM_CAMS = 527480, 871


def problems():
    def bal871():
        sizes, ss, _, _ = T.gen_bal_synthetic()
        sol = B.create_solver(B.Settings(), sizes, ss, [0, NUM_PTS])
        pt, cam = (0, NUM_PTS), (NUM_PTS, NUM_PTS + NUM_CAMS)
        return sol, {"camera-camera": (cam, cam), "point-camera": (pt, cam)}

    def grid82():
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
        sol = B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)
        return sol, {"any": ((0, ss.order()), (0, ss.order()))}

    return {"grid82": grid82, "bal871": bal871}


def solve_route(sol, L, pairs, sizes, max_cols):
    """what the library allowed before: unit columns, solve() over all of them, a gather; chunked like
    inverseBlocks so that the right-hand sides hold at most max_cols x order values"""
    import torch
    n = sol.order()
    perm = sol.scalarPermutation()
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]  # caller's scalar index of every param
    out = []
    k0 = 0
    while k0 < len(pairs):
        prm, cols, k1 = {}, 0, k0
        while k1 < len(pairs):
            new = [p for p in set(pairs[k1]) if p not in prm]
            add = sum(int(sizes[p]) for p in new)
            if k1 > k0 and cols + add > max_cols:
                break
            for p in new:
                prm[p] = cols
                cols += int(sizes[p])
            k1 += 1
        X = torch.zeros((cols, n), dtype=L.dtype, device=L.device)
        rows = np.concatenate([perm[first[p]] + np.arange(sizes[p]) for p in prm])
        X[torch.arange(cols, device=L.device), torch.from_numpy(rows).to(L.device)] = 1.0
        sol.solve(L, X, stride=n, nRHS=cols)
        for p, q in pairs[k0:k1]:
            rp = torch.from_numpy(perm[first[p]] + np.arange(sizes[p])).to(L.device)
            out.append(X[prm[q]:prm[q] + int(sizes[q])].index_select(1, rp).t())
        k0 = k1
    return out


def timed(fn, warmup, reps):
    import torch
    ms = []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="grid82,bal871")
    ap.add_argument("--pairs", default="16,128,1024")
    ap.add_argument("--skip-solve-route-above", type=int, default=0,
                    help="do not time the solve() route for more pairs than this (0: always time it)")
    a = ap.parse_args()
    import torch
    for name in a.only.split(","):
        sol, kinds = problems()[name]()
        sizes = np.diff(sol.skel()["spanStart"])[sol.paramToSpan()]
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        src = torch.from_numpy(h).to("cuda")
        L = src.clone()
        fac_ms, _ = timed(lambda: (L.copy_(src), sol.factor(L)), a.warmup, a.reps)
        Z = L.clone()
        sel_ms, _ = timed(lambda: (Z.copy_(L), sol.selectedInverse(Z)), a.warmup, a.reps)
        plan = sol._testReachPlan([0])
        print(json.dumps({"problem": name, "order": sol.order(), "lumps": sol.numLumps(), "cutLump": plan["cutLump"],
                          "scalars_behind_the_cut": sol.order() - int(sol.skel()["lumpStart"][plan["cutLump"]]),
                          "factor_ms": round(fac_ms, 3), "copy_plus_selected_inverse_ms": round(sel_ms, 3)}), flush=True)
        rng = np.random.default_rng(37)
        for kind, ((r0, r1), (c0, c1)) in kinds.items():
            for npairs in [int(x) for x in a.pairs.split(",")]:
                pairs = list(zip(rng.integers(r0, r1, npairs).tolist(), rng.integers(c0, c1, npairs).tolist()))
                on = 0
                for p, q in pairs:
                    try:
                        sol.blockOffset(p, q)
                        on += 1
                    except RuntimeError:
                        pass
                reach_ms, got = timed(lambda: sol.inverseBlocks(L, pairs), a.warmup, a.reps)
                rec = {"problem": name, "pairs": kind, "num_pairs": npairs, "on_the_pattern_of_L": on,
                       "distinct_columns": int(sum(sizes[p] for p in {p for pq in pairs for p in pq})),
                       "inverse_blocks_ms": round(reach_ms, 3), "selected_inverse_ms": round(sel_ms, 3),
                       "inverse_blocks_over_factor": round(reach_ms / fac_ms, 2)}
                if a.skip_solve_route_above == 0 or npairs <= a.skip_solve_route_above:
                    solve_ms, want = timed(lambda: solve_route(sol, L, pairs, sizes, sol.INVERSE_BLOCKS_MAX_COLUMNS),
                                           a.warmup, a.reps)
                    diff = max(float((g - w).abs().max()) for g, w in zip(got, want))
                    rec.update(solve_route_ms=round(solve_ms, 3), solve_route_over_inverse_blocks=round(solve_ms / reach_ms, 2),
                               max_abs_difference=diff)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
