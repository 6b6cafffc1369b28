"""GPU: log-determinant, pattern gradient and the autograd functions built on them
(Solver.logDet / Solver.patternGrad / baspacho_amd.autograd).
logDet is checked against numpy's slogdet, patternGrad against the numpy statement of
autograd_ref.py, and the autograd functions against torch's dense autograd through
cholesky / cholesky_solve / logdet of the matrix gathered from `data` (which encodes the
conventions by construction), plus gradcheck, batches, streams, run counters and sync freedom."""
import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import autograd as BA
from autograd_ref import element_coords, pattern_grad_ref, torch_dense
from helpers import solver_random, spd_data, to_dev
from selinv_cases import build_case, case_names

pytestmark = pytest.mark.gpu

LOGDET_TOL = {np.float64: 1e-12, np.float32: 1e-5}


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _structure(name):
    if name == "random":
        return solver_random(81, find_ranges=False)[0]
    if name == "random_ranges":
        return solver_random(82)[0]
    if name == "elim_range":
        return solver_random(83, fill=0.05, elim=(0, 40), ranges=[0, 40])[0]
    return build_case(name)[0]


STRUCTURES = ["random", "random_ranges", "elim_range"] + case_names()


# ---- logDet ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", STRUCTURES)
def test_logdet_matches_slogdet(name, dtype):
    sol = _structure(name)
    data = spd_data(sol, 7, dtype=dtype)
    sign, want = np.linalg.slogdet(sol.densify(data.astype(np.float64), fill_upper_half=True))
    assert sign > 0
    L = to_dev(data)
    sol.factor(L)
    got = sol.logDet(L)
    assert got.dtype == L.dtype and got.shape == () and got.is_cuda
    assert abs(float(got) - want) <= LOGDET_TOL[dtype] * abs(want), (float(got), want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_logdet_bitwise_and_batch(dtype):
    sol = _structure("elim_range")
    Ls = [to_dev(spd_data(sol, 20 + q, dtype=dtype)) for q in range(5)]
    sol.factor(Ls)
    singles = [sol.logDet(L) for L in Ls]
    again = [sol.logDet(L) for L in Ls]
    batch = sol.logDet(Ls)
    assert batch.shape == (5,)
    for q in range(5):
        assert torch.equal(_bits(singles[q]), _bits(again[q]))
        assert torch.equal(_bits(singles[q]), _bits(batch[q]))


def test_logdet_nonpositive_pivot_propagates():
    sol = _structure("random")
    L = to_dev(spd_data(sol, 3))
    sol.factor(L)
    off, _ = sol.diagBlockOffsetOfSpan(0)
    Ln = L.clone()
    Ln[off] = -1.0
    assert torch.isnan(sol.logDet(Ln))
    Ln[off] = 0.0
    assert float(sol.logDet(Ln)) == -np.inf


def test_logdet_70000_members_past_grid_limit():
    """members are 'factors' whose diagonal is c_q times the base's: log det = base + 2 n log c_q"""
    sol = build_case("width17")[0]
    n, ds, nb = sol.order(), sol.dataSize(), 70000
    base = to_dev(spd_data(sol, 9))
    sol.factor(base)
    ref = float(sol.logDet(base))
    c = 1.0 + torch.arange(nb, dtype=torch.float64, device="cuda") / nb
    X = base[None, :] * c[:, None]
    got = sol.logDet(list(X.unbind(0)))
    want = ref + 2 * n * torch.log(c)
    assert got.shape == (nb,)
    assert torch.allclose(got, want, rtol=1e-12, atol=0), (got - want).abs().max()


# ---- patternGrad -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 3, 16, 17])
@pytest.mark.parametrize("name", ["random", "elim_range", "width65", "small/at_all_limits"])
def test_pattern_grad_matches_reference(name, k, dtype):
    sol = _structure(name)
    coords = element_coords(sol)
    i, j = coords
    n, ds = sol.order(), sol.dataSize()
    rng = np.random.default_rng(k)
    U = rng.standard_normal((n, k)).astype(dtype)
    V = rng.standard_normal((n, k)).astype(dtype)
    Z = rng.standard_normal(ds).astype(dtype)
    ld = n + 5  # a leading dimension larger than n
    Ud = torch.zeros((k, ld), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    Vd = torch.zeros_like(Ud)
    Ud[:, :n] = to_dev(U.T)
    Vd[:, :n] = to_dev(V.T)
    s = to_dev(np.array([0.75], dtype=dtype))
    tol = 1e-13 if dtype == np.float64 else 1e-5
    cases = [("uv", dict(U=Ud, V=Vd), dict(U=U, V=V, alpha=-1.5)),
             ("z", dict(Z=to_dev(Z), zScale=s), dict(Z=Z, s=0.75)),
             ("both", dict(Z=to_dev(Z), zScale=s, U=Ud, V=Vd), dict(Z=Z, s=0.75, U=U, V=V, alpha=-1.5))]
    for what, kw, ref_kw in cases:
        out = torch.full((ds,), float("nan"), dtype=Ud.dtype, device="cuda")
        alpha = ref_kw.get("alpha", 1.0)
        sol.patternGrad(out, nRHS=k, alpha=alpha, stride=ld, **kw)
        got = out.cpu().numpy().astype(np.float64)
        want = pattern_grad_ref(sol, coords=coords, **{a: (b.astype(np.float64) if isinstance(b, np.ndarray) else b)
                                                      for a, b in ref_kw.items()})
        assert not np.isnan(got).any(), what
        assert np.all(got[i < j] == 0), what
        scale = np.abs(want).max()
        assert np.abs(got - want).max() <= tol * scale * max(k, 1), (what, np.abs(got - want).max(), scale)


def test_pattern_grad_batch_is_bitwise_single():
    sol = _structure("elim_range")
    n, ds, nb, k = sol.order(), sol.dataSize(), 4, 3
    g = torch.Generator(device="cuda").manual_seed(3)
    U = torch.randn((nb, k, n), dtype=torch.float64, device="cuda", generator=g)
    V = torch.randn((nb, k, n), dtype=torch.float64, device="cuda", generator=g)
    Z = torch.randn((nb, ds), dtype=torch.float64, device="cuda", generator=g)
    s = torch.tensor([0.5, -1.0, 2.0, 3.0], dtype=torch.float64, device="cuda")
    out = torch.full((nb, ds), float("nan"), dtype=torch.float64, device="cuda")
    sol.patternGrad(list(out.unbind(0)), Z=list(Z.unbind(0)), zScale=s, U=list(U.unbind(0)),
                    V=list(V.unbind(0)), nRHS=k, alpha=-1.0)
    for q in range(nb):
        one = torch.full((ds,), float("nan"), dtype=torch.float64, device="cuda")
        sol.patternGrad(one, Z=Z[q], zScale=s[q:q + 1], U=U[q], V=V[q], nRHS=k, alpha=-1.0)
        assert torch.equal(_bits(one), _bits(out[q])), q


def test_pattern_grad_refuses_bad_arguments():
    sol = _structure("random")
    ds, n = sol.dataSize(), sol.order()
    out = torch.zeros(ds, dtype=torch.float64, device="cuda")
    U = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="nothing to compute"):
        sol.patternGrad(out)
    with pytest.raises(RuntimeError, match="together"):
        sol.patternGrad(out, U=U)
    with pytest.raises(RuntimeError, match="nRHS"):
        sol.patternGrad(out, U=U, V=U, nRHS=0)
    with pytest.raises(RuntimeError, match="scale"):
        sol.patternGrad(out, Z=out)


# ---- autograd ----------------------------------------------------------------------------------------
def _dense_ref(sol, coords, data, b=None):
    """(x, logdet) through torch's dense autograd on A gathered from data"""
    A = torch_dense(data, coords)
    C = torch.linalg.cholesky(A)
    ld = 2 * torch.log(torch.diagonal(C, dim1=-2, dim2=-1)).sum(-1)
    if b is None:
        return None, ld
    bb = b.unsqueeze(-1) if b.dim() == A.dim() - 1 else b
    x = torch.cholesky_solve(bb, C)
    return x.reshape(b.shape), ld


def _inputs(sol, batch=None, k=None, dtype=torch.float64, seed=0):
    n = sol.order()
    if batch is None:
        d = to_dev(spd_data(sol, 40 + seed)).to(dtype)
    else:
        d = torch.stack([to_dev(spd_data(sol, 40 + seed + q)) for q in range(batch)]).to(dtype)
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = ((batch,) if batch else ()) + (n,) + ((k,) if k else ())
    b = torch.randn(shape, dtype=torch.float64, device="cuda", generator=g).to(dtype)
    w = torch.randn(shape, dtype=torch.float64, device="cuda", generator=g).to(dtype)
    return d, b, w


def _run(fn, sol, d, b, w):
    """loss value and gradients (data, b) of fn in {'solve', 'logdet', 'solve_logdet'}"""
    d = d.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    if fn == "solve":
        x = BA.solve(sol, d, b)
        loss = (w * x).sum()
    elif fn == "logdet":
        loss = BA.logdet(sol, d).sum()
    else:
        x, ld = BA.solve_logdet(sol, d, b)
        loss = (w * x).sum() + 0.5 * ld.sum()
    loss.backward()
    return loss.detach(), d.grad, b.grad


def _run_dense(fn, sol, coords, d, b, w):
    d = d.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    x, ld = _dense_ref(sol, coords, d, None if fn == "logdet" else b)
    if fn == "solve":
        loss = (w * x).sum()
    elif fn == "logdet":
        loss = ld.sum()
    else:
        loss = (w * x).sum() + 0.5 * ld.sum()
    loss.backward()
    gb = b.grad if b.grad is not None else None
    return loss.detach(), d.grad, gb


def _close(a, b, rtol):
    scale = b.abs().max().clamp_min(1e-300)
    return float((a - b).abs().max() / scale) <= rtol


FUNCS = ["solve", "logdet", "solve_logdet"]


@pytest.mark.parametrize("k", [None, 3])
@pytest.mark.parametrize("fn", FUNCS)
@pytest.mark.parametrize("name", ["random", "elim_range", "width65", "mixed_owners"])
def test_autograd_matches_dense_fp64(name, fn, k):
    sol = _structure(name)
    coords = element_coords(sol)
    d, b, w = _inputs(sol, k=k)
    d0 = d.clone()
    loss, gd, gb = _run(fn, sol, d, b, w)
    rloss, rgd, rgb = _run_dense(fn, sol, coords, d, b, w)
    assert torch.equal(d, d0)
    assert _close(loss, rloss, 1e-11)
    assert not torch.isnan(gd).any()
    assert _close(gd, rgd, 1e-10), float((gd - rgd).abs().max())
    i, j = coords
    assert torch.all(gd[torch.as_tensor(i < j, device="cuda")] == 0)
    if fn == "logdet":
        assert gb is None
    else:
        assert _close(gb, rgb, 1e-10)


@pytest.mark.parametrize("fn", FUNCS)
def test_autograd_fp32_loose(fn):
    sol = _structure("elim_range")
    coords = element_coords(sol)
    d, b, w = _inputs(sol, k=2)
    loss, gd, gb = _run(fn, sol, d.float(), b.float(), w.float())
    rloss, rgd, rgb = _run_dense(fn, sol, coords, d, b, w)
    assert gd.dtype == torch.float32
    x, ld = _dense_ref(sol, coords, d, b)  # (the loss of solve may cancel: bound it by its terms)
    scale = (w.abs() * x.abs()).sum() + ld.abs()
    assert float((loss.double() - rloss).abs()) <= 1e-5 * float(scale)
    assert _close(gd.double(), rgd, 1e-3)
    if gb is not None:
        assert _close(gb.double(), rgb, 1e-3)


@pytest.mark.parametrize("k", [None, 2])
@pytest.mark.parametrize("fn", FUNCS)
def test_autograd_batch_equals_loop(fn, k):
    sol = _structure("elim_range")
    d, b, w = _inputs(sol, batch=3, k=k)
    loss, gd, gb = _run(fn, sol, d, b, w)
    parts = [_run(fn, sol, d[q], b[q], w[q]) for q in range(3)]
    assert torch.allclose(loss, sum(p[0] for p in parts), rtol=1e-12)
    for q in range(3):
        assert torch.allclose(gd[q], parts[q][1], rtol=1e-12, atol=1e-15)
        if gb is not None:
            assert torch.allclose(gb[q], parts[q][2], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", ["small/n17_k1", "small/n1_17_chains", "tiny_random"])
def test_gradcheck(name):
    sol = solver_random(84, size=8, fill=0.2)[0] if name == "tiny_random" else _structure(name)
    assert sol.dataSize() < 1000
    d, b, _ = _inputs(sol, k=2)
    d.requires_grad_(True)
    b.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda dd, bb: BA.solve(sol, dd, bb), (d, b))
    assert torch.autograd.gradcheck(lambda dd: BA.logdet(sol, dd), (d,))
    assert torch.autograd.gradcheck(lambda dd, bb: BA.solve_logdet(sol, dd, bb), (d, b))


# ---- paths ---------------------------------------------------------------------------------------------
def _chunks(sol):
    torch.cuda.synchronize()
    return sol.runCounters()["selinv_chunks"]


@pytest.mark.parametrize("batch", [None, 3])
def test_selinv_runs_only_for_logdet_backward(batch):
    sol = _structure("elim_range")
    d, b, w = _inputs(sol, batch=batch)
    d.requires_grad_(True)
    b.requires_grad_(True)
    c0 = _chunks(sol)
    x = BA.solve(sol, d, b)
    (w * x).sum().backward()
    assert _chunks(sol) == c0
    ld = BA.logdet(sol, d)
    assert _chunks(sol) == c0
    ld.sum().backward()
    assert _chunks(sol) == c0 + 1
    x, ld = BA.solve_logdet(sol, d, b)
    (w * x).sum().backward()  # the log-determinant is not used: no selected inversion
    assert _chunks(sol) == c0 + 1


def test_retain_graph_and_double_backward():
    sol = _structure("elim_range")
    d, b, w = _inputs(sol)
    d.requires_grad_(True)
    b.requires_grad_(True)
    x, ld = BA.solve_logdet(sol, d, b)
    loss = (w * x).sum() + ld
    g1 = torch.autograd.grad(loss, (d, b), retain_graph=True)
    g2 = torch.autograd.grad(loss, (d, b), retain_graph=True)
    # the saved factor is intact; solve()'s atomics allow rounding-level differences in lambda
    for a, c in zip(g1, g2):
        assert torch.allclose(a, c, rtol=1e-13, atol=1e-13 * float(a.abs().max()))
    gd, = torch.autograd.grad(loss, d, create_graph=True)
    with pytest.raises(RuntimeError):
        gd.sum().backward()


def test_non_default_stream_and_solver_stream_restored():
    sol = _structure("elim_range")
    coords = element_coords(sol)
    d, b, w = _inputs(sol, k=2)
    ref = _run_dense("solve_logdet", sol, coords, d, b, w)
    own = torch.cuda.Stream()
    sol.setStream(own)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = _run("solve_logdet", sol, d, b, w)
    s.synchronize()
    assert sol._stream is own
    sol.setStream(None)
    assert _close(got[0], ref[0], 1e-11)
    assert _close(got[1], ref[1], 1e-10) and _close(got[2], ref[2], 1e-10)


def test_no_host_sync_after_warmup():
    sol = _structure("elim_range")
    for batch in (None, 2):
        d, b, w = _inputs(sol, batch=batch, k=2)
        _run("solve_logdet", sol, d, b, w)  # warm-up: plans and scratch
        torch.cuda.synchronize()
        d.requires_grad_(True)
        b.requires_grad_(True)
        torch.cuda.set_sync_debug_mode("error")
        try:
            x, ld = BA.solve_logdet(sol, d, b)
            ((w * x).sum() + ld.sum()).backward()
            x = BA.solve(sol, d, b)
            (w * x).sum().backward()
            BA.logdet(sol, d).sum().backward()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()


def test_incomplete_factor_solver_refused():
    sol, _, _ = solver_random(61, fill=0.03, elim=(0, 60), ranges=[0, 60], policy=B.AddFillForGivenElims)
    assert sol.canFactorUpToSpan() < sol.numSpans()
    d = torch.zeros(sol.dataSize(), dtype=torch.float64, device="cuda")
    b = torch.zeros(sol.order(), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="complete factor"):
        BA.solve(sol, d, b)
    with pytest.raises(ValueError, match="complete factor"):
        BA.logdet(sol, d)
    with pytest.raises(RuntimeError, match="complete factor"):
        sol.logDet(d)
    with pytest.raises(RuntimeError, match="complete factor"):
        sol.patternGrad(d, U=b[None], V=b[None])
