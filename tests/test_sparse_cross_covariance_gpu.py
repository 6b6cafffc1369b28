"""GPU: sparse.cross_covariance and sparse.joint_covariance (entries of A^-1 on and off the pattern, by
reach solves) against dense numpy / torch on the CPU.

A random pattern of order 120 in the caller's order, as test_sparse_covariance_gpu.py builds it: params of
sizes 1..4, full diagonal blocks, random off-diagonal blocks, duplicate entries.  Values against
np.linalg.inv in correlation units |got - want| / sqrt(want_ii want_jj), at least half of the pairs off
the pattern (asserted); gradients against torch.linalg.inv autograd on the dense matrix."""
import numpy as np
import pytest
import torch

from baspacho_amd import sparse as S
from helpers import to_dev

pytestmark = pytest.mark.gpu

# values: as test_inverse_blocks_gpu.py (10x the worst value of the first MI355X run over both files:
# fp64 1.33e-15, fp32 7.68e-7; this file's own worst: 6.4e-16 and 2.7e-7)
TOL = {torch.float64: 1.33e-14, torch.float32: 7.7e-6}
# gradients: relative to the largest reference gradient; the matrix has cond < 100 (asserted).  fp64: the
# 1e-10 and fp32: the 1e-4 of the other gradient tests of these layers (test_sparse_marginalize_gpu.py,
# test_partial_adjoint_gpu.py); about 840 fp32 eps, for a gradient that goes through two solves and a
# product at cond < 100
GRAD_TOL = {torch.float64: 1e-10, torch.float32: 1e-4}
N = 120


def _problem(seed):
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
    order = rng.permutation(len(rows))
    rows, cols = rows[order], cols[order]
    v = rng.uniform(-1, 1, len(rows)) * 0.3
    v[rows == cols] = rng.uniform(4, 6, int((rows == cols).sum()))
    pat = S.SymmetricPattern(rows, cols, N, param_sizes=ps)
    return pat, rows, cols, v, st


def _dense(rows, cols, values):
    A = torch.zeros(N, N, dtype=torch.float64).index_put((torch.as_tensor(rows), torch.as_tensor(cols)), values,
                                                         accumulate=True)
    return torch.tril(A) + torch.tril(A, -1).T


def _off_pattern(rows, cols, i, j):
    """which scalar pairs are no entry of the pattern, in either orientation: what covariance() cannot give"""
    have = set((rows * N + cols).tolist())
    return np.array([(max(a, b) * N + min(a, b)) not in have for a, b in zip(i.tolist(), j.tolist())])


@pytest.fixture(scope="module")
def problem():
    pat, rows, cols, v, st = _problem(3)
    assert len(rows) > len(np.unique(rows * N + cols)), "no duplicates"
    rng = np.random.default_rng(21)
    i, j = rng.integers(0, N, 400), rng.integers(0, N, 400)
    i[:5], j[:5] = [0, 7, 7, N - 1, 30], [0, 7, 7, 0, 30]  # diagonal entries, a repeated pair, a far pair
    off = _off_pattern(rows, cols, i, j)
    assert 2 * int(off.sum()) >= len(i), "fewer than half of the pairs are off the pattern"
    return pat, rows, cols, v, i, j


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cross_covariance_values_and_gradients(problem, dtype):
    pat, rows, cols, v, i, j = problem
    v = v.astype(np.float32).astype(np.float64) if dtype == torch.float32 else v
    rng = np.random.default_rng(9)
    w = rng.uniform(-1, 1, len(i))
    vt = torch.tensor(v, requires_grad=True)
    A = _dense(rows, cols, vt)
    assert np.linalg.cond(A.detach().numpy()) < 100
    C = torch.linalg.inv(A)
    (torch.as_tensor(w) * C[torch.as_tensor(i), torch.as_tensor(j)]).sum().backward()
    Cn = np.linalg.inv(A.detach().numpy())
    d = np.diag(Cn)
    g_ref = vt.grad.numpy()

    vd = to_dev(v).to(dtype).requires_grad_(True)
    stream_before = pat.solver._stream
    c = S.cross_covariance(pat, vd, i, j)
    assert c.shape == (len(i),) and c.dtype == dtype
    (to_dev(w).to(dtype) * c).sum().backward()
    assert pat.solver._stream is stream_before
    e_val = float((np.abs(c.detach().cpu().numpy().astype(np.float64) - Cn[i, j]) / np.sqrt(d[i] * d[j])).max())
    e_g = float(np.abs(vd.grad.cpu().numpy().astype(np.float64) - g_ref).max() / np.abs(g_ref).max())
    print("invblk-err sparse-cross %s %.3e" % (str(dtype).split(".")[-1], e_val))
    print("cross-grad %s %.3e" % (str(dtype).split(".")[-1], e_g))
    assert e_val < TOL[dtype]
    assert e_g < GRAD_TOL[dtype]
    # a second run: bitwise the same values and gradients
    v2 = to_dev(v).to(dtype).requires_grad_(True)
    c2 = S.cross_covariance(pat, v2, i, j)
    (to_dev(w).to(dtype) * c2).sum().backward()
    assert torch.equal(c2.detach(), c.detach()) and torch.equal(v2.grad, vd.grad)


def test_backward_in_chunks(problem, monkeypatch):
    """more pairs than one patternGrad call of the backward takes: the partial gradients are added"""
    pat, rows, cols, v, i, j = problem
    w = np.random.default_rng(4).uniform(-1, 1, len(i))
    grads = []
    for chunk in (256, 64):
        monkeypatch.setattr(S, "_CROSS_BACKWARD_CHUNK", chunk)
        vd = to_dev(v).requires_grad_(True)
        (to_dev(w) * S.cross_covariance(pat, vd, i, j)).sum().backward()
        grads.append(vd.grad.cpu().numpy())
    assert len(i) > 256
    assert np.abs(grads[0] - grads[1]).max() < GRAD_TOL[torch.float64] * np.abs(grads[0]).max()


def test_joint_covariance(problem):
    pat, rows, cols, v, _, _ = problem
    idx = np.array([5, 119, 0, 64, 63, 17, 90])
    vt = torch.tensor(v, requires_grad=True)
    C = torch.linalg.inv(_dense(rows, cols, vt))
    J_ref = C[torch.as_tensor(idx)][:, torch.as_tensor(idx)]
    w = torch.as_tensor(np.random.default_rng(2).uniform(-1, 1, (len(idx), len(idx))))
    (w * J_ref).sum().backward()
    vd = to_dev(v).requires_grad_(True)
    J = S.joint_covariance(pat, vd, idx)
    assert J.shape == (len(idx), len(idx))
    assert torch.equal(J, J.t())
    torch.linalg.cholesky(J.detach())
    (w.cuda() * J).sum().backward()
    d = np.sqrt(np.diag(J_ref.detach().numpy()))
    e_val = float((np.abs(J.detach().cpu().numpy() - J_ref.detach().numpy()) / np.outer(d, d)).max())
    e_g = float(np.abs(vd.grad.cpu().numpy() - vt.grad.numpy()).max() / np.abs(vt.grad.numpy()).max())
    print("invblk-err sparse-joint float64 %.3e" % e_val)
    print("joint-grad float64 %.3e" % e_g)
    assert e_val < TOL[torch.float64] and e_g < GRAD_TOL[torch.float64]


def test_arguments_are_checked_as_solve_checks_them(problem):
    pat, rows, cols, v, i, j = problem
    for fn, args in ((S.cross_covariance, (i, j)), (S.joint_covariance, (i[:4],))):
        with pytest.raises(TypeError):
            fn(pat, v, *args)  # not a tensor
        with pytest.raises(ValueError):
            fn(pat, to_dev(v[:-1]), *args)  # wrong length
        with pytest.raises(ValueError):
            fn(pat, torch.as_tensor(v), *args)  # host memory
        with pytest.raises(TypeError):
            fn(pat.solver, to_dev(v), *args)  # not a pattern
        with pytest.raises(ValueError, match="one matrix at a time"):
            fn(pat, to_dev(np.stack([v, v])), *args)  # a batch
    with pytest.raises(ValueError):
        S.cross_covariance(pat, to_dev(v), [0, N], [0, 0])  # a scalar out of range
    with pytest.raises(ValueError):
        S.cross_covariance(pat, to_dev(v), [0, 1], [0])  # lengths differ
    assert S.cross_covariance(pat, to_dev(v), [], []).shape == (0,)
