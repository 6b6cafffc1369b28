"""GPU: the normal equations of a sparse Jacobian on the MI355X.  hessian,
hessianAdjoint, jtVec and jVec must be bitwise the numpy restatement (normal_eq_ref.py) in f64 and f32 on
every case, into outputs full of NaN; batch members bitwise the single call, across the 65535 chunk
limit; baspacho_amd.sparse's lstsq / normal_equations / hessian / marginalize must match dense float64
torch in value and gradient at the bounds the other sparse tests use (1e-10 in f64, 1e-4 in f32), pass
gradcheck, give identical bits on a side stream, and refuse bad arguments before device work."""
import ctypes

import numpy as np
import pytest
import torch

from baspacho_amd import sparse as S
import normal_eq_ref as R

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
TOL = {"f64": dict(rtol=1e-10, atol=1e-10), "f32": dict(rtol=1e-4, atol=1e-4)}
SOLVABLE = ["scalar", "blocks", "blocks_elim", "hub"]  # J^T J >= 4 I


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _nan(shape, tdt):
    return torch.full(shape, float("nan"), dtype=tdt, device="cuda")


def _dev(a, npdt):
    return torch.from_numpy(np.ascontiguousarray(a.astype(npdt))).cuda()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", R.CASES)
def test_hessian_bitwise(case, dt):
    tdt, npdt = DT[dt]
    c, pat = R.pattern(case)
    table, _ = R.reference(case)
    sol, ne = pat.solver, pat.normal_eq
    out = _nan((sol.dataSize(),), tdt)
    got = ne.hessian(_dev(c["values"], npdt), out=out)
    assert got is out
    got = got.cpu().numpy()
    assert _bits_equal(got, R.ref_hessian(sol, table, c["values"], npdt))
    sp = sol.scalarPermutation()
    dense = sol.densify(got.astype(np.float64), fill_upper_half=True)[np.ix_(sp, sp)]
    J = R.dense_j(c["m"], c["n"], c["rows"], c["cols"], c["values"].astype(npdt).astype(np.float64))
    np.testing.assert_allclose(dense, J.T @ J, rtol=1e-5 if dt == "f32" else 1e-13, atol=1e-5 if dt == "f32" else 1e-13)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", R.CASES)
def test_adjoint_and_vectors_bitwise(case, dt):
    tdt, npdt = DT[dt]
    c, pat = R.pattern(case)
    _, terms = R.reference(case)
    sol, ne, rows, cols, m, n = pat.solver, pat.normal_eq, c["rows"], c["cols"], c["m"], c["n"]
    rng = np.random.default_rng(21)
    v = _dev(c["values"], npdt)
    gd = rng.uniform(-1, 1, sol.dataSize())
    out = _nan((len(rows),), tdt)
    ne.hessianAdjoint(v, _dev(gd, npdt), out=out)
    assert _bits_equal(out.cpu().numpy(), R.ref_adjoint(terms, len(rows), c["values"], gd, npdt))
    for q in (None, 1, 3):
        r = rng.uniform(-1, 1, (m,) if q is None else (m, q))
        x = rng.uniform(-1, 1, (n,) if q is None else (n, q))
        g = ne.jtVec(v, _dev(r, npdt), out=_nan((n,) + r.shape[1:], tdt))
        assert _bits_equal(g.cpu().numpy(), R.ref_jt_vec(rows, cols, n, c["values"], r, npdt))
        y = ne.jVec(v, _dev(x, npdt), out=_nan((m,) + x.shape[1:], tdt))
        assert _bits_equal(y.cpu().numpy(), R.ref_j_vec(rows, cols, m, c["values"], x, npdt))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_members_bitwise(dt):
    tdt, npdt = DT[dt]
    c, pat = R.pattern("hub")
    sol, ne, m, n = pat.solver, pat.normal_eq, c["m"], c["n"]
    rng = np.random.default_rng(22)
    vals = _dev(rng.uniform(-1, 1, (3, len(c["rows"]))), npdt)
    gd = _dev(rng.uniform(-1, 1, (3, sol.dataSize())), npdt)
    r = _dev(rng.uniform(-1, 1, (3, m, 2)), npdt)
    x = _dev(rng.uniform(-1, 1, (3, n)), npdt)
    H = ne.hessian(vals, out=_nan((3, sol.dataSize()), tdt))
    gv = ne.hessianAdjoint(vals, gd, out=_nan(tuple(vals.shape), tdt))
    g = ne.jtVec(vals, r, out=_nan((3, n, 2), tdt))
    y = ne.jVec(vals, x, out=_nan((3, m), tdt))
    for b in range(3):
        one = vals[b].clone()
        assert torch.equal(ne.hessian(one), H[b])
        assert torch.equal(ne.hessianAdjoint(one, gd[b].clone()), gv[b])
        assert torch.equal(ne.jtVec(one, r[b].clone()), g[b])
        assert torch.equal(ne.jVec(one, x[b].clone()), y[b])


def test_batch_past_chunk_limit():
    c, pat = R.pattern("one")
    ne, batch = pat.normal_eq, 65537
    vals = torch.rand(batch, 1, dtype=torch.float32, device="cuda")
    gd = torch.rand(batch, 1, dtype=torch.float32, device="cuda")
    H = ne.hessian(vals, out=_nan((batch, 1), torch.float32))
    assert torch.equal(H, vals * vals)
    gv = ne.hessianAdjoint(vals, gd, out=_nan((batch, 1), torch.float32))
    assert torch.equal(gv, gd * vals + gd * vals)
    assert torch.equal(ne.jtVec(vals, gd, out=_nan((batch, 1), torch.float32)), vals * gd)
    assert torch.equal(ne.jVec(vals, gd, out=_nan((batch, 1), torch.float32)), vals * gd)
    for b in (0, 65534, 65535, batch - 1):
        assert torch.equal(ne.hessian(vals[b].clone()), H[b])


# ---- baspacho_amd.sparse ---------------------------------------------------------------------------
def _dense_problem(c, v, r, alpha, beta):
    """x = (J^T J + D)^-1 J^T r by dense float64 torch on the CPU, differentiable"""
    rows, cols = torch.from_numpy(c["rows"]), torch.from_numpy(c["cols"])
    J = torch.zeros(c["m"], c["n"], dtype=torch.float64).index_put((rows, cols), v)
    H = J.T @ J
    H = H + torch.diag(torch.diagonal(H) * alpha + beta)
    return H, J.T @ r


def _leaves(c, dt, q, seed):
    rng = np.random.default_rng(seed)
    tdt, npdt = DT[dt]
    v = c["values"].astype(npdt)
    r = rng.uniform(-1, 1, (c["m"], q) if q else (c["m"],)).astype(npdt)
    w = rng.uniform(-1, 1, (c["n"], q) if q else (c["n"],)).astype(npdt)
    return v, r, w


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [0, 2])
@pytest.mark.parametrize("case", SOLVABLE)
def test_lstsq_matches_dense_autograd(case, q, dt):
    c, pat = R.pattern(case)
    v, r, w = _leaves(c, dt, q, 23)
    cpu = [torch.tensor(a.astype(np.float64), requires_grad=True) for a in (v, r, np.float64(0.3), np.float64(0.7))]
    H, g = _dense_problem(c, *cpu)
    xd = torch.linalg.solve(H, g)
    (xd * torch.from_numpy(w.astype(np.float64))).sum().backward()
    dev = [torch.tensor(a, device="cuda", requires_grad=True) for a in (v, r, v.dtype.type(0.3), v.dtype.type(0.7))]
    x = S.lstsq(pat, dev[0], dev[1], damping=(dev[2], dev[3]))
    assert x.shape == xd.shape and x.dtype == DT[dt][0]
    (x * torch.from_numpy(w).cuda()).sum().backward()
    torch.testing.assert_close(x.detach().cpu().double(), xd.detach(), **TOL[dt])
    for name, a, b in zip(("jvalues", "r", "alpha", "beta"), dev, cpu):
        torch.testing.assert_close(a.grad.cpu().double(), b.grad, msg=lambda m: "%s: %s" % (name, m), **TOL[dt])
    # float damping and none
    H0, g0 = _dense_problem(c, cpu[0].detach(), cpu[1].detach(), 0.0, 0.0)
    x0 = S.lstsq(pat, dev[0].detach(), dev[1].detach())
    torch.testing.assert_close(x0.cpu().double(), torch.linalg.solve(H0, g0), **TOL[dt])
    x1 = S.lstsq(pat, dev[0].detach(), dev[1].detach(), damping=(0.3, 0.7))
    torch.testing.assert_close(x1.cpu().double(), xd.detach(), **TOL[dt])


def test_normal_equations_and_hessian_against_dense():
    c, pat = R.pattern("blocks")
    v, r, _ = _leaves(c, "f64", 0, 24)
    vd = torch.tensor(v, device="cuda", requires_grad=True)
    rd = torch.tensor(r, device="cuda", requires_grad=True)
    beta = torch.tensor(0.5, dtype=torch.float64, device="cuda", requires_grad=True)
    data, g = S.normal_equations(pat, vd, rd, damping=(0.0, beta))
    assert torch.equal(data, S.hessian(pat, vd, damping=(0.0, beta))) and torch.equal(g, S.jt_vec(pat, vd, rd))
    assert torch.equal(S.hessian(pat, vd), pat.normal_eq.hessian(vd.detach()))
    sol, sp = pat.solver, pat.solver.scalarPermutation()
    W = np.random.default_rng(25).uniform(-1, 1, sol.dataSize())
    ((data * torch.from_numpy(W).cuda()).sum() + g.sum()).backward()
    vc, rc, bc = (torch.tensor(a, requires_grad=True) for a in (v, r, np.float64(0.5)))
    H, gc = _dense_problem(c, vc, rc, 0.0, bc)
    torch.testing.assert_close(g.detach().cpu(), gc.detach(), **TOL["f64"])
    dense = sol.densify(data.detach().cpu().numpy(), fill_upper_half=True)[np.ix_(sp, sp)]
    np.testing.assert_allclose(dense, H.detach().numpy(), rtol=1e-13, atol=1e-13)
    # the weight of dense H_ij in the loss: section 13's convention folds W onto the lower triangle
    Wd = np.tril(sol.densify(W))
    Wd = torch.from_numpy((Wd + np.tril(Wd, -1).T)[np.ix_(sp, sp)])
    ((torch.tril(H) * torch.tril(Wd)).sum() + gc.sum()).backward()
    for a, b in ((vd, vc), (rd, rc), (beta, bc)):
        torch.testing.assert_close(a.grad.cpu(), b.grad, **TOL["f64"])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_marginalize_on_a_jacobian_pattern(dt):
    c, pat = R.pattern("blocks_keep")
    keep, rest = c["keep"], np.setdiff1d(np.arange(c["n"]), c["keep"])
    v, r, _ = _leaves(c, dt, 2, 26)
    vc, rc = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (v, r))
    H, g = _dense_problem(c, vc, rc, 0.0, 0.0)
    X = torch.linalg.solve(H[np.ix_(rest, rest)], torch.cat([H[np.ix_(rest, keep)], g[rest]], dim=1))
    Sd = H[np.ix_(keep, keep)] - H[np.ix_(keep, rest)] @ X[:, :len(keep)]
    rd = g[keep] - H[np.ix_(keep, rest)] @ X[:, len(keep):]
    rng = np.random.default_rng(27)
    W, w = rng.uniform(-1, 1, Sd.shape), rng.uniform(-1, 1, rd.shape)
    ((Sd * torch.from_numpy(W)).sum() + (rd * torch.from_numpy(w)).sum()).backward()
    vd, rdev = (torch.tensor(a, device="cuda", requires_grad=True) for a in (v, r))
    Sg, rg = S.marginalize(pat, vd, rdev)
    ((Sg * _dev(W, v.dtype)).sum() + (rg * _dev(w, v.dtype)).sum()).backward()
    rel = lambda a, b: float(np.linalg.norm(a.detach().cpu().double().numpy() - b.detach().numpy())
                             / np.linalg.norm(b.detach().numpy()))
    errs = [rel(Sg, Sd), rel(rg, rd), rel(vd.grad, vc.grad), rel(rdev.grad, rc.grad)]
    print("marginalize %s: S %.2e r %.2e dvalues %.2e dr %.2e" % ((dt,) + tuple(errs)))
    assert max(errs) < TOL[dt]["rtol"], errs
    only = S.marginalize(pat, vd.detach())
    assert rel(only, Sd) < TOL[dt]["rtol"]


def test_gradcheck():
    c, pat = R.pattern("scalar_small")
    v = torch.tensor(c["values"], device="cuda", requires_grad=True)
    r = torch.randn(c["m"], 2, dtype=torch.float64, device="cuda", requires_grad=True)
    x = torch.randn(c["n"], dtype=torch.float64, device="cuda", requires_grad=True)
    a = torch.tensor(0.2, dtype=torch.float64, device="cuda", requires_grad=True)
    b = torch.tensor(0.4, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v_, r_, a_, b_: S.lstsq(pat, v_, r_, damping=(a_, b_)), (v, r, a, b))
    assert torch.autograd.gradcheck(lambda v_, a_, b_: S.hessian(pat, v_, damping=(a_, b_)), (v, a, b))
    assert torch.autograd.gradcheck(lambda v_, r_: S.jt_vec(pat, v_, r_), (v, r))
    assert torch.autograd.gradcheck(lambda v_, x_: S.j_vec(pat, v_, x_), (v, x))


def test_batched_lstsq_matches_single():
    c, pat = R.pattern("scalar")
    rng = np.random.default_rng(28)
    vb = torch.from_numpy(np.stack([c["values"], c["values"] * 1.5, c["values"] * 0.75])).cuda().requires_grad_()
    rb = torch.from_numpy(rng.uniform(-1, 1, (3, c["m"]))).cuda()
    xb = S.lstsq(pat, vb, rb, damping=(0.1, 0.2))
    xb.sum().backward()
    for q in range(3):
        v1 = vb[q].detach().clone().requires_grad_()
        x = S.lstsq(pat, v1, rb[q], damping=(0.1, 0.2))
        x.sum().backward()
        torch.testing.assert_close(xb[q], x, **TOL["f64"])
        torch.testing.assert_close(vb.grad[q], v1.grad, **TOL["f64"])
        assert torch.equal(S.hessian(pat, vb)[q], S.hessian(pat, v1))


def test_on_side_stream():
    c, pat = R.pattern("blocks")
    v = torch.tensor(c["values"], device="cuda", requires_grad=True)
    r = torch.randn(c["m"], dtype=torch.float64, device="cuda", requires_grad=True)
    W = torch.randn(pat.solver.dataSize(), dtype=torch.float64, device="cuda")

    def run():
        data, g = S.normal_equations(pat, v, r, damping=(0.1, 0.2))
        y = S.j_vec(pat, v, g)
        gv, gr = torch.autograd.grad((data * W).sum() + g.sum() + y.sum(), (v, r))
        return data.detach(), g.detach(), y.detach(), gv, gr

    first = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        second = run()
    torch.cuda.current_stream().wait_stream(s)
    assert pat.solver._stream is None
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_no_host_sync():
    c, pat = R.pattern("scalar")
    v = torch.tensor(c["values"], device="cuda", requires_grad=True)
    r = torch.randn(c["m"], 2, dtype=torch.float64, device="cuda", requires_grad=True)
    S.lstsq(pat, v, r, damping=(0.1, 0.2)).sum().backward()  # first call: uploads the maps and the index arrays
    v.grad = r.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        S.lstsq(pat, v, r, damping=(0.1, 0.2)).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(v.grad).all() and torch.isfinite(r.grad).all()


def test_argument_errors_before_device_work():
    c, pat = R.pattern("scalar")
    sol, ne, m, n, nnz = pat.solver, pat.normal_eq, c["m"], c["n"], len(c["rows"])
    other = S.JacobianPattern(c["rows"], c["cols"], m, n).solver
    lib, P = sol._lib, ctypes.c_void_p
    vals = torch.rand(nnz, dtype=torch.float64, device="cuda")
    r = torch.rand(m, dtype=torch.float64, device="cuda")
    out = _nan((2, sol.dataSize()), torch.float64)
    gn = _nan((2, n), torch.float64)
    vp, rp, o0, o1, g0, g1 = (t.data_ptr() for t in (vals, r, out[0], out[1], gn[0], gn[1]))
    arr = lambda *p: (P * len(p))(*p)

    def err(rc):
        assert rc != 0
        return lib.bsp_last_error().decode()

    assert "another solver" in err(lib.bsp_normal_eq_hessian_f64(other._h, ne._h, P(vp), P(o0)))
    assert "values pointer of batch member 0 is NULL" in err(lib.bsp_normal_eq_hessian_f64(sol._h, ne._h, P(None), P(o0)))
    assert "data pointer of batch member 0 is NULL" in err(lib.bsp_normal_eq_hessian_f64(sol._h, ne._h, P(vp), P(None)))
    assert "batch is empty" in err(lib.bsp_normal_eq_hessian_batched_f64(sol._h, ne._h, arr(vp), arr(o0), 0))
    assert "NULL" in err(lib.bsp_normal_eq_hessian_batched_f64(sol._h, ne._h, None, arr(o0), 1))
    assert "repeats" in err(lib.bsp_normal_eq_hessian_batched_f64(sol._h, ne._h, arr(vp, vp), arr(o0, o0), 2))
    assert "batch member 1 is NULL" in err(lib.bsp_normal_eq_hessian_batched_f64(sol._h, ne._h, arr(vp, None), arr(o0, o1), 2))
    assert "aliases its values" in err(lib.bsp_normal_eq_hessian_f64(sol._h, ne._h, P(o0), P(o0 + 8)))
    assert "aliases its gradient-of-data" in err(lib.bsp_normal_eq_hessian_adjoint_f64(sol._h, ne._h, P(vp), P(o0), P(o0)))
    assert "another solver" in err(lib.bsp_normal_eq_hessian_adjoint_batched_f64(other._h, ne._h, arr(vp), arr(o0), arr(o1), 1))
    q1 = ctypes.c_int64(1)
    assert "vector pointer of batch member 0 is NULL" in err(lib.bsp_normal_eq_jt_vec_f64(sol._h, ne._h, P(vp), P(None), q1, P(g0)))
    assert "at least one" in err(lib.bsp_normal_eq_jt_vec_f64(sol._h, ne._h, P(vp), P(rp), ctypes.c_int64(0), P(g0)))
    assert "repeats" in err(lib.bsp_normal_eq_jt_vec_batched_f64(sol._h, ne._h, arr(vp, vp), arr(rp, rp), q1, arr(g0, g0), 2))
    assert "also an output" in err(lib.bsp_normal_eq_j_vec_batched_f64(sol._h, ne._h, arr(vp, vp), arr(g0, o0), q1, arr(o0, o1), 2))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(gn).all()  # nothing was written
    with pytest.raises(ValueError):
        ne.hessian(vals[:-1])
    with pytest.raises(ValueError):
        ne.hessian(vals, out=out)
    with pytest.raises(ValueError, match="empty batch"):
        ne.hessian(vals.reshape(1, -1)[:0])
    with pytest.raises(TypeError):
        ne.hessian(vals.to(torch.int64))
    with pytest.raises(TypeError):
        ne.jtVec(vals, r.float())
    with pytest.raises(ValueError):
        ne.jtVec(vals, r[:-1])
    with pytest.raises(ValueError, match="device memory"):
        S.lstsq(pat, vals.cpu(), r.cpu())
    with pytest.raises(TypeError, match="dtype"):
        S.lstsq(pat, vals, r.float())
    with pytest.raises(ValueError, match="rows"):
        S.lstsq(pat, vals, torch.ones(m + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="empty batch"):
        S.hessian(pat, vals.reshape(1, -1)[:0])
    with pytest.raises(TypeError, match="JacobianPattern"):
        S.lstsq(S.SymmetricPattern([0], [0], 1), vals, r)
    with pytest.raises(ValueError, match="0-dim"):
        S.hessian(pat, vals, damping=(torch.ones(2, dtype=torch.float64, device="cuda"), 0.0))
