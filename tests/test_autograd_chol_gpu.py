"""GPU: baspacho_amd.autograd.cholesky / solve_l / solve_lt and sparse.sample against dense torch
autograd (torch.linalg.cholesky / solve_triangular in fp64), single and batched, one and several
right-hand sides, fp64 and fp32; retain_graph, streams, and the log-determinant through the factor."""
import numpy as np
import pytest
import torch

from baspacho_amd import autograd as BA
from baspacho_amd import sparse as S
from autograd_ref import element_coords, torch_dense
from known_factor import known_factor_data
from selinv_cases import build_case

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-10, torch.float32: 2e-4}


def _problem(dtype, batch, seed=3):
    sol, _ = build_case("mixed_owners")
    rows = [known_factor_data(sol, seed + q, np.float64, rho=0.5).data for q in range(max(batch, 1))]
    d = torch.tensor(np.stack(rows) if batch else rows[0], dtype=dtype, device="cuda")
    return sol, d, element_coords(sol)


def _dense_L(d64, coords):
    return torch.linalg.cholesky(torch_dense(d64, coords))


def _gather(Ld, coords):
    i, j = coords
    return Ld[..., torch.as_tensor(i, device=Ld.device), torch.as_tensor(j, device=Ld.device)]


def _close(a, b, tol):
    a, b = a.double(), b.double()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err < tol, err


def _rhs(sol, batch, k, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    shape = ((batch,) if batch else ()) + (sol.order(),) + ((k,) if k else ())
    return torch.rand(shape, generator=g, dtype=torch.float64).mul_(2).sub_(1).to("cuda", dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("batch", [0, 3])
def test_cholesky_against_dense(dtype, batch):
    sol, d, coords = _problem(dtype, batch)
    i, j = coords
    W = torch.rand(d.shape, dtype=torch.float64, device="cuda") * torch.as_tensor(i >= j, device="cuda")
    d1 = d.clone().requires_grad_(True)
    L = BA.cholesky(sol, d1)
    assert torch.equal(d1.detach(), d), "the forward modified its input"
    (W.to(dtype) * L).sum().backward()
    d2 = d.double().clone().requires_grad_(True)
    L2 = _gather(_dense_L(d2, coords), coords)
    (W * L2).sum().backward()
    _close(L.detach(), L2.detach(), TOL[dtype])
    assert (L.detach()[..., torch.as_tensor(i < j, device="cuda")] == 0).all()
    _close(d1.grad, d2.grad, TOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("batch", [0, 2])
@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("which", ["l", "lt"])
def test_half_solves_against_dense(which, k, batch, dtype):
    sol, d, coords = _problem(dtype, batch, seed=9)
    b = _rhs(sol, batch, k, dtype, 1)
    wy = _rhs(sol, batch, k, torch.float64, 2)
    fn = BA.solve_l if which == "l" else BA.solve_lt
    d1, b1 = d.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = fn(sol, BA.cholesky(sol, d1), b1)
    assert torch.equal(b1.detach(), b)
    (wy.to(dtype) * y).sum().backward()
    d2, b2 = d.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    Ld = _dense_L(d2, coords)
    bb = b2 if k else b2.unsqueeze(-1)
    if which == "l":
        y2 = torch.linalg.solve_triangular(Ld, bb, upper=False)
    else:
        y2 = torch.linalg.solve_triangular(Ld.transpose(-1, -2), bb, upper=True)
    y2 = y2 if k else y2.squeeze(-1)
    (wy * y2).sum().backward()
    _close(y.detach(), y2.detach(), TOL[dtype])
    _close(d1.grad, d2.grad, TOL[dtype])
    _close(b1.grad, b2.grad, TOL[dtype])


def test_retain_graph_runs_a_second_backward():
    sol, d, _ = _problem(torch.float64, 0)
    b = _rhs(sol, 0, 2, torch.float64, 4)
    d1, b1 = d.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss = (BA.solve_lt(sol, BA.cholesky(sol, d1), b1) ** 2).sum()
    loss.backward(retain_graph=True)
    g1, h1 = d1.grad.clone(), b1.grad.clone()
    loss.backward()
    # the half-solves accumulate with atomics (hip_solve_kernels.h): close, not bitwise
    _close(d1.grad, 2 * g1, 1e-12)
    _close(b1.grad, 2 * h1, 1e-12)


def test_callers_stream_is_used_and_solver_stream_restored():
    sol, d, _ = _problem(torch.float64, 0)
    b = _rhs(sol, 0, 0, torch.float64, 5)
    ref_d = d.clone().requires_grad_(True)
    (BA.solve_l(sol, BA.cholesky(sol, ref_d), b) ** 2).sum().backward()
    side = torch.cuda.Stream()
    sol.setStream(None)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d1 = d.clone().requires_grad_(True)
        (BA.solve_l(sol, BA.cholesky(sol, d1), b) ** 2).sum().backward()
    assert sol._stream is None
    torch.cuda.current_stream().wait_stream(side)
    _close(d1.grad, ref_d.grad, 1e-12)


@pytest.mark.parametrize("batch", [0, 2])
def test_log_sum_of_diagonal_matches_logdet(batch):
    sol, d, (i, j) = _problem(torch.float64, batch, seed=12)
    diag = torch.as_tensor(np.nonzero(i == j)[0], device="cuda")
    d1 = d.clone().requires_grad_(True)
    ld1 = 2 * BA.cholesky(sol, d1)[..., diag].log().sum(-1)
    ld1.sum().backward()
    d2 = d.clone().requires_grad_(True)
    ld2 = BA.logdet(sol, d2)
    ld2.sum().backward()
    _close(ld1.detach(), ld2.detach(), 1e-12)
    _close(d1.grad, d2.grad, 1e-10)


# ---- sparse.sample ---------------------------------------------------------------------------
def _entries(n, seed):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, n, 3 * n)
    c = rng.integers(0, n, 3 * n)
    lo, hi = np.maximum(r, c), np.minimum(r, c)
    keep = lo != hi
    rows = np.concatenate([np.arange(n), lo[keep]])
    cols = np.concatenate([np.arange(n), hi[keep]])
    vals = np.concatenate([rng.uniform(4.0, 6.0, n), rng.uniform(-0.5, 0.5, int(keep.sum()))])
    return rows, cols, vals


def _dense_user(rows, cols, vals, n):
    A = torch.zeros(vals.shape[:-1] + (n, n), dtype=vals.dtype, device=vals.device)
    flat = A.reshape(vals.shape[:-1] + (n * n,))
    r = torch.as_tensor(rows, device=vals.device)
    c = torch.as_tensor(cols, device=vals.device)
    low = flat.index_add(-1, r * n + c, vals).reshape(A.shape)
    return low + low.transpose(-1, -2) - torch.diag_embed(torch.diagonal(low, dim1=-2, dim2=-1))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("batch", [0, 2])
@pytest.mark.parametrize("k", [0, 4])
def test_sample_against_dense(k, batch, dtype):
    n = 70
    rows, cols, vals = _entries(n, 7)
    pat = S.SymmetricPattern(rows, cols, n)
    v = torch.tensor(np.stack([vals * (1 + 0.1 * q) for q in range(max(batch, 1))]) if batch else vals,
                     dtype=dtype, device="cuda")
    z = _rhs(pat.solver, batch, k, dtype, 8)
    mu = _rhs(pat.solver, batch, k, dtype, 9)
    w = _rhs(pat.solver, batch, k, torch.float64, 10)
    v1, z1, m1 = (t.clone().requires_grad_(True) for t in (v, z, mu))
    x = S.sample(pat, v1, z1, m1)
    (w.to(dtype) * x).sum().backward()
    v2, z2, m2 = (t.double().clone().requires_grad_(True) for t in (v, z, mu))
    inv = torch.as_tensor(pat._to_internal, device="cuda")
    perm = torch.as_tensor(pat._to_user, device="cuda")
    A = _dense_user(rows, cols, v2, n)
    Ai = A[..., inv, :][..., :, inv]
    Ld = torch.linalg.cholesky(Ai)
    zz = z2 if k else z2.unsqueeze(-1)
    xi = torch.linalg.solve_triangular(Ld.transpose(-1, -2), zz.index_select(-2, inv), upper=True)
    x2 = xi.index_select(-2, perm)
    x2 = m2 + (x2 if k else x2.squeeze(-1))
    (w * x2).sum().backward()
    _close(x.detach(), x2.detach(), TOL[dtype])
    for a, b in ((v1, v2), (z1, z2), (m1, m2)):
        _close(a.grad, b.grad, TOL[dtype])


def test_sample_covariance_is_the_inverse():
    """Cov(x) = A^-1: x x^T averaged over the columns of an identity z is exactly A^-1 / n"""
    n = 40
    rows, cols, vals = _entries(n, 3)
    pat = S.SymmetricPattern(rows, cols, n)
    v = torch.tensor(vals, dtype=torch.float64, device="cuda")
    X = S.sample(pat, v, torch.eye(n, dtype=torch.float64, device="cuda"))
    A = _dense_user(rows, cols, v, n)
    _close(X @ X.T, torch.linalg.inv(A), 1e-12)
