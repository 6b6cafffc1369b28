"""GPU: sparse.marginalize against dense numpy A22 - A21 A11^-1 A12 and b2 - A21 A11^-1 b1 in the order
of `keep` (keep shuffled, params of mixed sizes, duplicate entries), its gradients against dense torch
on the CPU, and inv(S) = the keep block of inv(A) against selectedInverse + marginals.  Bounds as
test_partial_adjoint_gpu.py: 1e-10 (fp64) and 1e-4 (fp32) relative to the largest reference value."""
import numpy as np
import pytest
import torch

from baspacho_amd import sparse as S
from chol_adjoint_ref import rel_error
from helpers import to_dev
from marginalize_cases import dense, random_problem, spd_values

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}


def _pattern(prob):
    return S.SymmetricPattern(prob["rows"], prob["cols"], prob["n"], param_sizes=prob["param_sizes"],
                              keep=prob["keep"])


def _split(prob):
    keep = prob["keep"]
    rest = np.setdiff1d(np.arange(prob["n"]), keep)
    return rest, keep


def _dense_torch(prob, values, b):
    """(S, r) by dense torch in fp64 on the CPU, differentiable in values and b"""
    n = prob["n"]
    rows, cols = torch.as_tensor(prob["rows"]), torch.as_tensor(prob["cols"])
    A = torch.zeros(n, n, dtype=torch.float64).index_put((rows, cols), values, accumulate=True)
    A = torch.tril(A) + torch.tril(A, -1).T
    rest, keep = (torch.as_tensor(x) for x in _split(prob))
    A11, A21, A22 = A[rest][:, rest], A[keep][:, rest], A[keep][:, keep]
    X = torch.linalg.solve(A11, torch.cat([A21.T, b[rest].reshape(len(rest), -1)], 1))
    Sd = A22 - A21 @ X[:, :len(keep)]
    r = b[keep].reshape(len(keep), -1) - A21 @ X[:, len(keep):]
    return Sd, r.reshape((len(keep),) + tuple(b.shape[1:]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("k", [0, 3])
def test_marginalize_values_and_gradients(seed, dtype, k):
    prob = random_problem(seed)
    pat = _pattern(prob)
    n, m = prob["n"], len(prob["keep"])
    v = spd_values(prob, seed, dtype)
    assert np.linalg.cond(dense(prob, v)) < 100
    rng = np.random.default_rng(seed + 10)
    b = rng.uniform(-1, 1, (n, k) if k else (n,)).astype(dtype)
    W = rng.uniform(-1, 1, (m, m)).astype(dtype)
    w = rng.uniform(-1, 1, (m, k) if k else (m,)).astype(dtype)
    vt = torch.tensor(v.astype(np.float64), requires_grad=True)
    bt = torch.tensor(b.astype(np.float64), requires_grad=True)
    Sd, rd = _dense_torch(prob, vt, bt)
    ((torch.as_tensor(W.astype(np.float64)) * Sd).sum() + (torch.as_tensor(w.astype(np.float64)) * rd).sum()).backward()
    for batch in (0, 3):
        rep = (lambda a: np.stack([a] * batch)) if batch else (lambda a: a)
        vd = to_dev(rep(v)).requires_grad_(True)
        bd = to_dev(rep(b)).requires_grad_(True)
        Sg, rg = S.marginalize(pat, vd, bd)
        assert Sg.shape == vd.shape[:-1] + (m, m) and rg.shape == vd.shape[:-1] + w.shape
        ((to_dev(W) * Sg).sum() + (to_dev(w) * rg).sum()).backward()
        only = S.marginalize(pat, vd.detach())
        # without b: the same S from a factor of its own (factor() is not bitwise reproducible: its
        # elimination updates add with atomics)
        assert rel_error(only.cpu().numpy(), Sg.detach().cpu().numpy()) < TOL[dtype]
        for q in range(max(batch, 1)):
            pick = (lambda t: t[q]) if batch else (lambda t: t)
            errs = [rel_error(pick(Sg).detach().cpu().numpy(), Sd.detach().numpy()),
                    rel_error(pick(rg).detach().cpu().numpy(), rd.detach().numpy()),
                    rel_error(pick(vd.grad).cpu().numpy(), vt.grad.numpy()),
                    rel_error(pick(bd.grad).cpu().numpy(), bt.grad.numpy())]
            print("seed %d k %d batch %d member %d: S %.2e r %.2e dvalues %.2e db %.2e" % ((seed, k, batch, q) + tuple(errs)))
            assert max(errs) < TOL[dtype], errs


def test_inverse_of_s_is_the_keep_block_of_the_inverse():
    """the identity that makes the marginal useful: inv(S) equals the keep rows / columns of inv(A);
    its diagonal param blocks against selectedInverse + marginals of the same pattern"""
    prob = random_problem(3)
    pat = _pattern(prob)
    sol = pat.solver
    v = spd_values(prob, 3)
    vd = to_dev(v)
    Sg = S.marginalize(pat, vd).cpu().numpy()
    C = np.linalg.inv(Sg)
    keep = prob["keep"]
    want = np.linalg.inv(dense(prob, v))[np.ix_(keep, keep)]
    assert rel_error(C, want) < 1e-10
    Z = S.assemble(pat, vd).clone()
    sol.factor(Z)
    sol.selectedInverse(Z)
    blocks = sol.marginals(Z, [int(p) for p in prob["keep_params"]])
    st = np.concatenate([[0], np.cumsum(prob["param_sizes"])])
    pos = {int(s): t for t, s in enumerate(keep)}
    for p, blk in zip(prob["keep_params"], blocks):
        idx = [pos[int(s)] for s in range(st[p], st[p + 1])]
        assert rel_error(C[np.ix_(idx, idx)], blk.cpu().numpy()) < 1e-10, int(p)
