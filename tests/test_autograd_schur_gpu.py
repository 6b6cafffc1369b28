"""GPU: autograd through the partial factor (baspacho_amd.autograd.factor_up_to / schur_complement /
solve_l_up_to) against dense torch autograd on the CPU of the same loss.
Data and bounds as test_partial_adjoint_gpu.py (1e-10 fp64, 1e-4 fp32, relative to max |grad|).

No host synchronisation inside the functions: checked by reading the code (as for cholesky in
test_autograd_chol_gpu.py's module: every step is a Solver call or a torch op on the current stream;
there is no .item(), .cpu() or synchronize in autograd.py)."""
import numpy as np
import pytest
import torch

from baspacho_amd import autograd as BA
from autograd_ref import element_coords, project
from chol_adjoint_ref import rel_error
from helpers import solver_random, to_dev
from kf_structures import bipartite, lump_over_lump
from known_factor import known_factor_data
from partial_adjoint_ref import bar_of, dense_partial_torch, splits
from selinv_cases import build_case

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}


def _cases():
    sol = bipartite(120, 7, 3, 6, seed=4)
    yield "bipartite", sol, int(sol.skel()["lumpToSpan"][int(sol.sparseEliminationRanges()[-1])])
    sol = lump_over_lump(300, 70)
    yield "lump_over_lump", sol, int(sol.skel()["lumpToSpan"][1])
    sol, _ = build_case("mixed_owners")
    sp = splits(sol)
    yield "mixed_owners", sol, sp[len(sp) // 2]
    sol, _, _ = solver_random(3, fill=0.037, elim=(0, 60))
    sp = splits(sol)
    yield "random3", sol, sp[len(sp) // 2]


def _dense_loss_grad(sol, data, span, W, w, b):
    """(data gradient, b gradient) of <W, S> + <w, y[bar:]>, y = [L11 0; L21 I]^-1 b, dense fp64 on the CPU"""
    coords = element_coords(sol)
    bar, n = bar_of(sol, span), sol.order()
    A = torch.tensor(sol.densify(np.asarray(data, dtype=np.float64), fill_upper_half=True), requires_grad=True)
    bt = torch.tensor(np.asarray(b, dtype=np.float64), requires_grad=True)
    P = dense_partial_torch(A, bar)
    S = A[bar:, bar:] - P[bar:, :bar] @ P[bar:, :bar].T if bar > 0 else A
    M = torch.cat([P[:, :bar], torch.cat([torch.zeros(bar, n - bar, dtype=A.dtype),
                                          torch.eye(n - bar, dtype=A.dtype)], 0)], 1)
    y = torch.linalg.solve_triangular(M, bt[:, None], upper=False)[:, 0]
    loss = (torch.as_tensor(np.asarray(W, dtype=np.float64)) * S).sum() + \
        (torch.as_tensor(np.asarray(w, dtype=np.float64)) * y[bar:]).sum()
    loss.backward()
    G = A.grad.numpy()
    return project(sol, 0.5 * (G + G.T), coords), bt.grad.numpy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_loss_gradient_against_dense_autograd(dtype):
    for name, sol, span in _cases():
        assert 0 < span < sol.numSpans()
        kf = known_factor_data(sol, 5, dtype, rho=0.5)
        assert np.linalg.cond(kf.A) < 100
        bar, n = bar_of(sol, span), sol.order()
        m = n - bar
        rng = np.random.default_rng(7)
        W = rng.uniform(-1, 1, (m, m)).astype(dtype)
        w = rng.uniform(-1, 1, m).astype(dtype)
        b = rng.uniform(-1, 1, n).astype(dtype)
        want_d, want_b = _dense_loss_grad(sol, kf.data, span, W, w, b)
        for batch in (0, 3):
            rep = (lambda a: np.stack([a] * batch)) if batch else (lambda a: a)
            data = to_dev(rep(kf.data)).requires_grad_(True)
            bd = to_dev(rep(b)).requires_grad_(True)
            S = BA.schur_complement(sol, data, span)
            P = BA.factor_up_to(sol, data, span)
            y = BA.solve_l_up_to(sol, P, span, bd)
            assert S.shape == data.shape[:-1] + (m, m)
            loss = (to_dev(W) * S).sum() + (to_dev(w) * y[..., bar:]).sum()
            loss.backward(retain_graph=True)
            g1, gb1 = data.grad.clone(), bd.grad.clone()
            data.grad = bd.grad = None
            loss.backward()
            for q in range(max(batch, 1)):
                gd = (g1[q] if batch else g1).cpu().numpy()
                gb = (gb1[q] if batch else gb1).cpu().numpy()
                ed, eb = rel_error(gd, want_d), rel_error(gb, want_b)
                print("%s batch %d member %d: data %.2e b %.2e" % (name, batch, q, ed, eb))
                assert ed < TOL[dtype] and eb < TOL[dtype], (name, batch, q, ed, eb)
            # a second backward over the retained graph: equal to rounding (the half-solves add with
            # atomics, so the order of their sums may differ: n eps with n <= 1000 scalars here)
            again = min(TOL[dtype], 1000 * float(np.finfo(dtype).eps))
            assert sol.order() <= 1000
            assert rel_error(data.grad.cpu().numpy(), g1.cpu().numpy()) < again
            assert rel_error(bd.grad.cpu().numpy(), gb1.cpu().numpy()) < again


def test_schur_complement_alone_is_bitwise_reproducible_and_symmetric():
    name, sol, span = next(_cases())
    kf = known_factor_data(sol, 5, np.float64, rho=0.5)
    bar = bar_of(sol, span)
    m = sol.order() - bar
    data = to_dev(kf.data).requires_grad_(True)
    S = BA.schur_complement(sol, data, span)
    A = kf.A
    want = A[bar:, bar:] - A[bar:, :bar] @ np.linalg.solve(A[:bar, :bar], A[:bar, bar:])
    assert rel_error(S.detach().cpu().numpy(), want) < 1e-10
    assert torch.equal(S, S.T)
    W = to_dev(np.random.default_rng(1).uniform(-1, 1, (m, m)))
    loss = (W * S).sum()
    loss.backward(retain_graph=True)
    g1 = data.grad.clone()
    data.grad = None
    loss.backward()
    assert torch.equal(g1, data.grad)
    # a permuted output: dest[k] = m - 1 - k
    dest = torch.arange(m - 1, -1, -1, dtype=torch.int32, device="cuda")
    Sp = BA.schur_complement(sol, data.detach(), span, dest=dest)
    assert torch.equal(Sp, S.detach().flip(0, 1))


def test_argument_checks():
    name, sol, span = next(_cases())
    data = torch.zeros(sol.dataSize(), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="span"):
        BA.factor_up_to(sol, data, sol.numSpans() + 1)
    with pytest.raises(ValueError, match="no span behind"):
        BA.schur_complement(sol, data, sol.numSpans())
    ranges = [int(r) for r in sol.sparseEliminationRanges()]
    inside = int(sol.skel()["lumpToSpan"][(ranges[0] + ranges[-1]) // 2])
    with pytest.raises(ValueError, match="sparse-elimination"):
        BA.schur_complement(sol, data, inside)
    with pytest.raises(ValueError, match="device memory"):
        BA.factor_up_to(sol, data.cpu(), span)
