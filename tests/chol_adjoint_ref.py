"""Reference of the factor's reverse mode (Solver.factorAdjoint).

dense_grad: the oracle.  A(d) densified in internal order, torch.linalg.cholesky in fp64 on the CPU,
the vector-Jacobian product with Lbar placed on the dense lower triangle, projected onto the
elements with autograd_ref.project (G_ij + G_ji below the diagonal, G_ii on it, 0 above it).

recurrence: a numpy restatement of the node recurrence over the selected-inversion plan
(Solver._testSelInvPlan()), in place in one gradient buffer with the G storage the kernels use:
G_RR read by selinvZAddr's rule, a node's rows inside its own lump mirrored into the upper triangle
of the lump's diagonal block, then the final element-wise conversion."""
import numpy as np

from autograd_ref import element_coords, project


def lbar_random(sol, seed, dtype=np.float64):
    """a random Lbar in the solver's layout (uniform(-1, 1); the strictly-upper elements of the
    diagonal blocks hold values too, which the adjoint must ignore)"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, sol.dataSize()).astype(dtype)


def dense_grad(sol, data, lbar, coords=None):
    """df/dd of f = <Lbar, L(d)> on the elements i >= j, from dense torch autograd in fp64"""
    import torch
    i, j = coords if coords is not None else element_coords(sol)
    A = torch.tensor(sol.densify(np.asarray(data, dtype=np.float64), fill_upper_half=True), requires_grad=True)
    L = torch.linalg.cholesky(A)
    low = i >= j
    Lb = torch.zeros_like(A)
    Lb[i[low], j[low]] = torch.as_tensor(np.asarray(lbar, dtype=np.float64)[low])
    (L * Lb).sum().backward()
    G = A.grad.numpy()
    return project(sol, 0.5 * (G + G.T), (i, j))


def dense_factor(sol, data):
    """the factor of A(d) in the layout (fp64, 0 on the strictly-upper elements)"""
    i, j = element_coords(sol)
    L = np.linalg.cholesky(sol.densify(np.asarray(data, dtype=np.float64), fill_upper_half=True))
    return L[i, j]


class _Layout:
    """lump columns of the layout: offset, width, global rows; element lookup by (row, col)"""

    def __init__(self, sol):
        sk = sol.skel()
        self.n = sol.order()
        self.ss = sk["spanStart"]
        rows, cols = element_coords(sol)
        self.key = rows * self.n + cols
        self.order = np.argsort(self.key)
        self.sorted = self.key[self.order]
        ls, cp, rte, cd = sk["lumpStart"], sk["chainColPtr"], sk["chainRowsTillEnd"], sk["chainData"]
        self.lumps = []
        for l in range(sol.numLumps()):
            w = int(ls[l + 1] - ls[l])
            off = int(cd[cp[l]])
            R = int(rte[cp[l + 1] - 1])
            self.lumps.append((off, w, R, rows[off + np.arange(R) * w]))

    def index(self, r, c):
        k = np.asarray(r) * self.n + np.asarray(c)
        p = np.searchsorted(self.sorted, k)
        assert (p < len(self.sorted)).all() and (self.sorted[np.minimum(p, len(self.sorted) - 1)] == k).all(), \
            "an element outside the stored pattern"
        return self.order[p]

    def span(self, r):
        return np.searchsorted(self.ss, r, side="right") - 1


def _zaddr(lay, gR, nRest):
    """element index of G(a, b) for every a, b of R, by selinvZAddr's rule"""
    r = len(gR)
    a = np.arange(r)[:, None]
    b = np.arange(r)[None, :]
    sa, sb = lay.span(gR)[:, None], lay.span(gR)[None, :]
    keep = (b < nRest) | ((a >= nRest) & (sa >= sb))  # read (row a, column b), else (row b, column a)
    rr = np.where(keep, gR[:, None], gR[None, :])
    cc = np.where(keep, gR[None, :], gR[:, None])
    return lay.index(rr, cc)


def _tri_inv(M):
    return np.linalg.inv(np.tril(M))


def recurrence_np(sol, L, lbar, plan=None):
    """numpy restatement of the node recurrence over the selected-inversion plan"""
    plan = plan if plan is not None else sol._testSelInvPlan()
    lay = _Layout(sol)
    Ld = np.asarray(L, dtype=np.float64)
    G = np.array(lbar, dtype=np.float64)
    recs = [(int(v), 0, k) for k, v in enumerate(plan["small"]["level"])]
    recs += [(int(v), 1, k) for k, v in enumerate(plan["node"]["level"])]
    for _, kind, k in sorted(recs):
        if kind == 0:
            sm = {f: int(plan["small"][f][k]) for f in plan["small"]}
            lump, c0, w, r, nRest = sm["lump"], 0, sm["n"], sm["r"], 0
        else:
            nd = {f: int(plan["node"][f][k]) for f in plan["node"]}
            lump, c0, w, r, nRest = nd["lump"], nd["c0"], nd["w"], nd["r"], nd["nRest"]
        off, lw, R, colRows = lay.lumps[lump]
        c1 = c0 + w
        assert R - c1 == r, (lump, R, c1, r)
        Lc = Ld[off:off + R * lw].reshape(R, lw)
        Gc = G[off:off + R * lw].reshape(R, lw)  # a view: writes go to G
        LII = np.tril(Lc[c0:c1, c0:c1])
        LRI = Lc[c1:, c0:c1]
        Linv = _tri_inv(LII)
        LbRI = Gc[c1:, c0:c1].copy()
        if r:
            GRR = G[_zaddr(lay, colRows[c1:], nRest)]
            LbRI -= 2.0 * GRR @ LRI                                     # 1
        Abar = LbRI @ Linv                                              # 2
        Gc[c1:, c0:c1] = 0.5 * Abar
        Gc[c0:c1, c1:c1 + nRest] = 0.5 * Abar[:nRest].T                 # the mirror
        LbII = np.tril(Gc[c0:c1, c0:c1]) - np.tril(Abar.T @ LRI)        # 3
        Phi = np.tril(LII.T @ LbII)
        Phi[np.diag_indices(w)] *= 0.5
        K = Linv.T @ Phi @ Linv                                         # 4
        Gc[c0:c1, c0:c1] = 0.5 * (K + K.T)
    i, j = element_coords(sol)
    return np.where(i > j, 2.0 * G, np.where(i == j, G, 0.0))


def rel_error(got, want):
    """max |got - want| / max |want|"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))
