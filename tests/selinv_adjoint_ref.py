"""Reference of selected inversion's reverse mode (Solver.selectedInverseAdjoint).

grad holds df/d(slot) for every slot of the layout as selectedInverse writes it: the strictly-upper
elements of the diagonal blocks are slots of their own (they hold Z_ji).  The result is Lbar = df/dL
on the elements i >= j and 0 above the diagonal.

dense_lbar: the oracle.  tril(L) densified in internal order, Z = inv(L L^T) by torch in fp64 on the
CPU, f = sum over the slots of grad * Z[i, j], the gradient of L gathered at element_coords.

zsz_projection: Abar = -proj(Z S Z) with S the symmetrised slot weights (the Jacobian of
A -> proj(A^-1) is self-adjoint), projected by autograd_ref.project: what the chain
factorAdjoint(L, selectedInverseAdjoint(L, Z, grad)) must give.

recurrence_np: a numpy restatement of the reverse sweep of the Takahashi recurrence over the
selected-inversion plan (Solver._testSelInvPlan()), descending level, in place in the gradient buffer
with selinvZAddr's addressing (chol_adjoint_ref._zaddr); every array in `dtype`."""
import numpy as np

from autograd_ref import element_coords, project
from chol_adjoint_ref import _Layout, _zaddr, rel_error  # noqa: F401  (rel_error: for the tests)


def grad_random(sol, seed, dtype=np.float64):
    """uniform(-1, 1) on every slot, mirrors included"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, sol.dataSize()).astype(dtype)


def dense_z(sol, L):
    """(A^-1 dense, selected inverse in the layout: every slot, mirrors included) of the factor L"""
    i, j = element_coords(sol)
    Ld = np.tril(sol.densify(np.asarray(L, dtype=np.float64)))
    Z = np.linalg.inv(Ld @ Ld.T)
    Z = 0.5 * (Z + Z.T)
    return Z, Z[i, j]


def dense_lbar(sol, L, grad, coords=None):
    """df/dL_e of f = sum_slots grad * inv(tril(L) tril(L)^T)[i, j] on i >= j (0 above), torch fp64"""
    import torch
    i, j = coords if coords is not None else element_coords(sol)
    Ld = torch.tensor(np.tril(sol.densify(np.asarray(L, dtype=np.float64))), requires_grad=True)
    Lt = torch.tril(Ld)
    Z = torch.linalg.inv(Lt @ Lt.T)
    w = torch.as_tensor(np.asarray(grad, dtype=np.float64))
    (Z[torch.as_tensor(i), torch.as_tensor(j)] * w).sum().backward()
    G = Ld.grad.numpy()
    return np.where(i >= j, G[i, j], 0.0)


def slot_weights(sol, grad, coords=None):
    """dense symmetric S: S_ij = S_ji = g_ij / 2 off the diagonal, S_ii = g_ii, g the sum of grad over
    the slots that hold Z_ij or Z_ji"""
    i, j = coords if coords is not None else element_coords(sol)
    n = sol.order()
    g = np.zeros((n, n))
    np.add.at(g, (i, j), np.asarray(grad, dtype=np.float64))
    return 0.5 * (g + g.T)


def zsz_projection(sol, L, grad, coords=None):
    """the projection of -Z S Z in section 13's convention"""
    coords = coords if coords is not None else element_coords(sol)
    Z, _ = dense_z(sol, L)
    return project(sol, -Z @ slot_weights(sol, grad, coords) @ Z, coords)


def recurrence_np(sol, L, Z, grad, plan=None, dtype=np.float64, scatter=True):
    """numpy restatement of the reverse sweep; scatter=False drops the scatter
    step (for the test that shows it is needed)"""
    plan = plan if plan is not None else sol._testSelInvPlan()
    lay = _Layout(sol)
    Ld = np.asarray(L, dtype=dtype)
    Zd = np.asarray(Z, dtype=dtype)
    G = np.array(grad, dtype=dtype)
    two, half = dtype(2), dtype(0.5)
    recs = [(int(v), 0, k) for k, v in enumerate(plan["small"]["level"])]
    recs += [(int(v), 1, k) for k, v in enumerate(plan["node"]["level"])]
    for _, kind, k in sorted(recs, reverse=True):
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
        Zc = Zd[off:off + R * lw].reshape(R, lw)
        Gc = G[off:off + R * lw].reshape(R, lw)  # a view: writes go to G
        Wi = np.linalg.inv(np.tril(Lc[c0:c1, c0:c1])).astype(dtype)
        g = Gc[c0:c1, c0:c1]
        SII = half * (g + g.T)
        Wbar = two * Wi @ SII
        if r:
            LRI = Lc[c1:, c0:c1]
            U = LRI @ Wi
            gRI = Gc[c1:, c0:c1].copy()
            gRI[:nRest] += Gc[c0:c1, c1:c1 + nRest].T          # fold the mirror
            SRI = half * gRI
            za = _zaddr(lay, colRows[c1:], nRest)
            if scatter:
                T = two * SRI - U @ SII
                D = -half * (T @ U.T + U @ T.T)
                np.add.at(G, za, D)
            Ubar = -two * (Zc[c1:, c0:c1] @ SII + Zd[za] @ SRI)
            Wbar = Wbar + LRI.T @ Ubar
            Gc[c1:, c0:c1] = Ubar @ Wi.T
            Gc[c0:c1, c1:c1 + nRest] = 0
        Gc[c0:c1, c0:c1] = -np.tril(Wi.T @ Wbar @ Wi.T)
    return G
