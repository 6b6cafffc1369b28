"""GPU: sparse.covariance and sparse.marginal_variances (entries of A^-1 on the pattern, through
selected inversion and its reverse mode) against dense numpy / torch on the CPU.

A random pattern of order 120 in the caller's order: params of sizes 1..4, full diagonal blocks, random
off-diagonal blocks, duplicate entries, "lower" and "full" (mirrored entries with row < col, which the
assembly skips).  The values give a diagonally dominant matrix with cond < 100 (asserted), so the
bounds are 1e-10 relative to the largest reference value, as for the other fp64 gradients of these
layers."""
import numpy as np
import pytest
import torch

from baspacho_amd import sparse as S
from chol_adjoint_ref import rel_error
from helpers import to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-10
N = 120


def _problem(seed, triangle):
    rng = np.random.default_rng(seed)
    ps = []
    while sum(ps) < N:
        ps.append(min(int(rng.integers(1, 5)), N - sum(ps)))
    ps = np.asarray(ps, dtype=np.int64)
    st = np.concatenate([[0], np.cumsum(ps)])
    rows, cols = [], []
    for p in range(len(ps)):
        for q in range(p + 1):
            if p == q or rng.random() < 0.06:
                for i in range(st[p], st[p + 1]):
                    for j in range(st[q], min(st[q + 1], i + 1)):
                        rows.append(i)
                        cols.append(j)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    dup = rng.choice(len(rows), size=len(rows) // 5, replace=False)  # duplicates: their values add up
    rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
    if triangle == "full":  # mirrors of some off-diagonal entries: skipped by the assembly
        mir = np.nonzero((rng.random(len(rows)) < 0.3) & (rows != cols))[0]
        rows, cols = np.concatenate([rows, cols[mir]]), np.concatenate([cols, rows[mir]])
    order = rng.permutation(len(rows))
    rows, cols = rows[order], cols[order]
    v = rng.uniform(-1, 1, len(rows)) * 0.3
    v[rows == cols] = rng.uniform(4, 6, int((rows == cols).sum()))
    pat = S.SymmetricPattern(rows, cols, N, param_sizes=ps, triangle=triangle)
    return pat, rows, cols, v


def _dense_torch(rows, cols, values):
    """(covariance at the entries with 0 for the skipped ones, diag(A^-1), A) by dense torch on the CPU"""
    kept = torch.as_tensor(rows >= cols)
    r, c = torch.as_tensor(rows), torch.as_tensor(cols)
    A = torch.zeros(N, N, dtype=torch.float64).index_put((r[kept], c[kept]), values[kept], accumulate=True)
    A = torch.tril(A) + torch.tril(A, -1).T
    C = torch.linalg.inv(A)
    return torch.where(kept, C[r, c], torch.zeros((), dtype=torch.float64)), torch.diagonal(C), A


@pytest.mark.parametrize("triangle", ["lower", "full"])
def test_covariance_and_variances_values_and_gradients(triangle):
    pat, rows, cols, v = _problem(3, triangle)
    skipped = rows < cols
    assert skipped.any() == (triangle == "full")
    assert len(rows) > len(np.unique(rows * N + cols)), "no duplicates"
    rng = np.random.default_rng(9)
    wc, wv = rng.uniform(-1, 1, len(rows)), rng.uniform(-1, 1, N)
    vt = torch.tensor(v, requires_grad=True)
    cov_ref, var_ref, A = _dense_torch(rows, cols, vt)
    assert np.linalg.cond(A.detach().numpy()) < 100
    ((torch.as_tensor(wc) * cov_ref).sum() + (torch.as_tensor(wv) * var_ref).sum()).backward()
    cov_ref, var_ref, g_ref = cov_ref.detach().numpy(), var_ref.detach().numpy(), vt.grad.numpy()
    zmax = np.abs(np.linalg.inv(A.detach().numpy())).max()

    vd = to_dev(v).requires_grad_(True)
    cov, var = S.covariance(pat, vd), S.marginal_variances(pat, vd)
    assert cov.shape == (len(rows),) and var.shape == (N,)
    ((to_dev(wc) * cov).sum() + (to_dev(wv) * var).sum()).backward()
    e_cov = float(np.abs(cov.detach().cpu().numpy() - cov_ref).max() / zmax)
    e_var = float(np.abs(var.detach().cpu().numpy() - var_ref).max() / zmax)
    e_g = rel_error(vd.grad.cpu().numpy(), g_ref)
    print("%s: covariance %.2e variances %.2e dvalues %.2e" % (triangle, e_cov, e_var, e_g))
    assert max(e_cov, e_var, e_g) < TOL
    # skipped entries: 0 and no gradient
    sk = torch.as_tensor(skipped, device="cuda")
    assert (cov.detach()[sk] == 0).all() and (vd.grad[sk] == 0).all()
    assert (g_ref[skipped] == 0).all()

    # a [3, nnz] batch against three single calls
    scale = np.array([1.0, 1.5, 0.75])[:, None]
    vb = to_dev(v[None, :] * scale).requires_grad_(True)
    cb, mb = S.covariance(pat, vb), S.marginal_variances(pat, vb)
    assert cb.shape == (3, len(rows)) and mb.shape == (3, N)
    ((to_dev(wc) * cb).sum() + (to_dev(wv) * mb).sum()).backward()
    for q in range(3):
        v1 = to_dev(v * scale[q]).requires_grad_(True)
        c1, m1 = S.covariance(pat, v1), S.marginal_variances(pat, v1)
        ((to_dev(wc) * c1).sum() + (to_dev(wv) * m1).sum()).backward()
        zq = zmax / scale[q, 0]
        assert float((cb[q] - c1).detach().abs().max()) / zq < TOL
        assert float((mb[q] - m1).detach().abs().max()) / zq < TOL
        assert rel_error(vb.grad[q].cpu().numpy(), v1.grad.cpu().numpy()) < TOL, q


def test_values_are_checked_as_solve_checks_them():
    pat, rows, cols, v = _problem(4, "lower")
    for fn in (S.covariance, S.marginal_variances):
        with pytest.raises(TypeError):
            fn(pat, v)  # not a tensor
        with pytest.raises(ValueError):
            fn(pat, to_dev(v[:-1]))  # wrong length
        with pytest.raises(ValueError):
            fn(pat, torch.as_tensor(v))  # host memory
        with pytest.raises(TypeError):
            fn(pat.solver, to_dev(v))  # not a pattern
