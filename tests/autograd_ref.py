"""Reference of the gradient conventions of baspacho_amd.autograd.

Every stored element e of the numeric layout sits at (row, col) = (i, j) of the dense matrix in the
solver's internal order.  A(d) has A_ij = A_ji = d_e for i >= j; the strictly-upper elements of the
diagonal blocks (i < j) are not read.  The gradient of the stored elements, from a dense gradient
G = df/dA, is G_ij + G_ji for i > j, G_ii for i = j and 0 for i < j."""
import numpy as np


def element_coords(sol):
    """(rows, cols) int64 arrays: the dense position of every element of the numeric layout"""
    sk = sol.skel()
    ls, ss = sk["lumpStart"], sk["spanStart"]
    rows = np.empty(sol.dataSize(), dtype=np.int64)
    cols = np.empty(sol.dataSize(), dtype=np.int64)
    for l in range(sol.numLumps()):
        c0, w = int(ls[l]), int(ls[l + 1] - ls[l])
        for c in range(int(sk["chainColPtr"][l]), int(sk["chainColPtr"][l + 1])):
            sp = int(sk["chainRowSpan"][c])
            r0, nr = int(ss[sp]), int(ss[sp + 1] - ss[sp])
            d0 = int(sk["chainData"][c])
            rr, cc = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + w), indexing="ij")
            rows[d0:d0 + nr * w] = rr.ravel()
            cols[d0:d0 + nr * w] = cc.ravel()
    return rows, cols


def project(sol, G, coords=None):
    """per-element gradient of the numeric layout from the dense gradient G (rules above)"""
    i, j = coords if coords is not None else element_coords(sol)
    out = G[i, j] + G[j, i]
    out[i == j] = G[i[i == j], j[i == j]]
    out[i < j] = 0
    return out


def pattern_grad_ref(sol, Z=None, s=1.0, U=None, V=None, alpha=1.0, coords=None):
    """numpy statement of Solver.patternGrad: U, V [n, k] (row = vector entry)"""
    i, j = coords if coords is not None else element_coords(sol)
    out = np.zeros(sol.dataSize())
    if U is not None:
        lo = np.einsum("ek,ek->e", U[i], V[j]) + np.einsum("ek,ek->e", V[i], U[j])
        dg = np.einsum("ek,ek->e", U[i], V[i])
        out += alpha * np.where(i == j, dg, lo)
    if Z is not None:
        out += s * np.where(i == j, 1.0, 2.0) * Z
    out[i < j] = 0
    return out


def torch_dense(data, coords):
    """A(data) as a dense torch matrix built by a differentiable gather of the i >= j elements;
    data [dataSize] or [B, dataSize]"""
    import torch
    i, j = coords
    keep = np.nonzero(i >= j)[0]
    ii = torch.as_tensor(i[keep], device=data.device)
    jj = torch.as_tensor(j[keep], device=data.device)
    kk = torch.as_tensor(keep, device=data.device)
    n = int(max(i.max(), j.max())) + 1
    vals = data[..., kk]
    L = torch.zeros(data.shape[:-1] + (n, n), dtype=data.dtype, device=data.device)
    L = _put(L, ii, jj, vals)
    return L + L.transpose(-1, -2) - torch.diag_embed(torch.diagonal(L, dim1=-2, dim2=-1))


def _put(L, ii, jj, vals):
    """L with vals at (ii, jj) (distinct positions), differentiable in vals"""
    flat = L.reshape(L.shape[:-2] + (-1,))
    n = L.shape[-1]
    flat = flat.index_add(-1, ii * n + jj, vals)
    return flat.reshape(L.shape)
