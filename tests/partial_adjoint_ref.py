"""Reference of the partial factor's reverse mode (Solver.factorAdjointUpTo).

oracle: dense torch autograd in fp64 on the CPU of P = [L11 0; L21 tril(S)], L11 = cholesky(A11),
L21 = A21 L11^-T, S = A22 - L21 L21^T, for f = <Pbar, P> with Pbar on the elements i >= j; projected
with autograd_ref.project.

recurrence_np: the numpy restatement of what the device runs: seed the trailing lumps (off-diagonal
elements halved, diagonal kept, diagonal blocks mirrored), the node recurrence of chol_adjoint_ref
over Solver._testSelInvPlan(span), the final element-wise conversion; with the kernels' addressing."""
import numpy as np

from autograd_ref import element_coords, project
from chol_adjoint_ref import _Layout, _tri_inv, _zaddr

MAX_SPLITS = 30


def bar_of(sol, span):
    return int(sol.skel()["spanStart"][span])


def splits(sol):
    """admissible cuts (the rule of test_partial_factor_gpu.admissible_splits): every lump boundary from
    the end of the last elimination range on, every range boundary, 0 and numSpans(); more than
    MAX_SPLITS: evenly sampled, the ends kept"""
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    dense_from = ranges[-1] if ranges else 0
    lumps = sorted(set(range(dense_from, sol.numLumps() + 1)) | set(ranges) | {0})
    spans = sorted({int(sol.skel()["lumpToSpan"][l]) for l in lumps})
    if len(spans) > MAX_SPLITS:
        idx = np.unique(np.round(np.linspace(0, len(spans) - 1, MAX_SPLITS)).astype(int))
        spans = [spans[t] for t in idx]
    assert spans[0] == 0 and spans[-1] == sol.numSpans()
    return spans


def dense_partial_torch(A, bar):
    """P = [L11 0; L21 tril(S)] of the dense symmetric torch matrix A"""
    import torch
    n = A.shape[0]
    if bar == 0:
        return torch.tril(A)
    L11 = torch.linalg.cholesky(A[:bar, :bar])
    if bar == n:
        return L11
    L21 = torch.linalg.solve_triangular(L11, A[bar:, :bar].T, upper=False).T
    S = A[bar:, bar:] - L21 @ L21.T
    top = torch.cat([L11, torch.zeros(bar, n - bar, dtype=A.dtype)], 1)
    return torch.cat([top, torch.cat([L21, torch.tril(S)], 1)], 0)


def oracle(sol, data, pbar, span, coords=None):
    """(df/dd of f = <Pbar, P(d)> on the elements i >= j, P in the layout with 0 above the diagonal)"""
    import torch
    i, j = coords if coords is not None else element_coords(sol)
    A = torch.tensor(sol.densify(np.asarray(data, dtype=np.float64), fill_upper_half=True), requires_grad=True)
    P = dense_partial_torch(A, bar_of(sol, span))
    low = i >= j
    Pb = torch.zeros_like(A)
    Pb[i[low], j[low]] = torch.as_tensor(np.asarray(pbar, dtype=np.float64)[low])
    (P * Pb).sum().backward()
    G = A.grad.numpy()
    return project(sol, 0.5 * (G + G.T), (i, j)), P.detach().numpy()[i, j]


def seed_np(sol, lay, G, cut_lump):
    """the trailing lumps of G from the data-gradient convention to G storage, in place"""
    for l in range(cut_lump, sol.numLumps()):
        off, lw, R, _ = lay.lumps[l]
        Gc = G[off:off + R * lw].reshape(R, lw)
        Gc[lw:, :] *= 0.5
        D = Gc[:lw, :lw].copy()
        low = 0.5 * np.tril(D, -1)
        Gc[:lw, :lw] = low + low.T + np.diag(np.diag(D))


def recurrence_np(sol, P, pbar, span, plan=None):
    """seed + the node recurrence over the plan of the cut + final conversion (fp64)"""
    plan = plan if plan is not None else sol._testSelInvPlan(span)
    cut = int(sol.skel()["spanToLump"][span]) if span < sol.numSpans() else sol.numLumps()
    lay = _Layout(sol)
    Ld = np.asarray(P, dtype=np.float64)
    G = np.array(pbar, dtype=np.float64)
    seed_np(sol, lay, G, cut)
    recs = [(int(v), 0, k) for k, v in enumerate(plan["small"]["level"])]
    recs += [(int(v), 1, k) for k, v in enumerate(plan["node"]["level"])]
    for _, kind, k in sorted(recs):
        if kind == 0:
            sm = {f: int(plan["small"][f][k]) for f in plan["small"]}
            lump, c0, w, r, nRest = sm["lump"], 0, sm["n"], sm["r"], 0
        else:
            nd = {f: int(plan["node"][f][k]) for f in plan["node"]}
            lump, c0, w, r, nRest = nd["lump"], nd["c0"], nd["w"], nd["r"], nd["nRest"]
        assert lump < cut, (lump, cut)
        off, lw, R, colRows = lay.lumps[lump]
        c1 = c0 + w
        assert R - c1 == r, (lump, R, c1, r)
        Lc = Ld[off:off + R * lw].reshape(R, lw)
        Gc = G[off:off + R * lw].reshape(R, lw)
        LII = np.tril(Lc[c0:c1, c0:c1])
        LRI = Lc[c1:, c0:c1]
        Linv = _tri_inv(LII)
        LbRI = Gc[c1:, c0:c1].copy()
        if r:
            LbRI -= 2.0 * G[_zaddr(lay, colRows[c1:], nRest)] @ LRI
        Abar = LbRI @ Linv
        Gc[c1:, c0:c1] = 0.5 * Abar
        Gc[c0:c1, c1:c1 + nRest] = 0.5 * Abar[:nRest].T
        LbII = np.tril(Gc[c0:c1, c0:c1]) - np.tril(Abar.T @ LRI)
        Phi = np.tril(LII.T @ LbII)
        Phi[np.diag_indices(w)] *= 0.5
        K = Linv.T @ Phi @ Linv
        Gc[c0:c1, c0:c1] = 0.5 * (K + K.T)
    i, j = element_coords(sol)
    return np.where(i > j, 2.0 * G, np.where(i == j, G, 0.0))


def plan_records(plan):
    """the records of a plan as a set of (lump, c0, w, r, nRest) and their levels by that key"""
    lev = {}
    sm, nd = plan["small"], plan["node"]
    for k in range(len(sm["lump"])):
        lev[(int(sm["lump"][k]), 0, int(sm["n"][k]), int(sm["r"][k]), 0)] = int(sm["level"][k])
    for k in range(len(nd["lump"])):
        lev[(int(nd["lump"][k]), int(nd["c0"][k]), int(nd["w"][k]), int(nd["r"][k]), int(nd["nRest"][k]))] = \
            int(nd["level"][k])
    return lev
