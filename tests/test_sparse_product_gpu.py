"""GPU: baspacho_amd.sparse's matvec, quad_form, log_prob and solve_refined on the
MI355X.  matvec against the dense product, its gradients against torch autograd on the dense matrix, both at
the bounds of a sequential sum; quad_form and log_prob against torch.distributions.MultivariateNormal in
value and gradient (1e-10 in f64, 1e-4 in f32, the bounds of the other sparse tests); solve_refined against
a longdouble-refined reference at 8 x the host model's own error (capped at 1e-13), at least 1000 times
closer than the fp32 solve, with gradients that match solve's in f64, on any stream."""
import numpy as np
import pytest
import torch

from baspacho_amd import sparse as S
import sym_product_ref as R

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
TOL = {"f64": dict(rtol=1e-10, atol=1e-10), "f32": dict(rtol=1e-4, atol=1e-4)}
# (batch, vectors): [n], [n, k], [B, n], [B, n, k]
SHAPES = [(None, None), (None, 3), (2, None), (3, 2)]


def _dense(c, v):
    """the dense matrix of the kept entries of case c from the torch values v ([nnz]), differentiable"""
    keep = c["rows"] >= c["cols"]
    idx = torch.from_numpy(np.nonzero(keep)[0])
    rows, cols = torch.from_numpy(c["rows"][keep]), torch.from_numpy(c["cols"][keep])
    L = torch.zeros(c["n"], c["n"], dtype=v.dtype).index_put_((rows, cols), v[idx], accumulate=True)
    return torch.tril(L) + torch.tril(L, -1).T


def _shape(n, nb, k):
    return (() if nb is None else (nb,)) + (n,) + (() if k is None else (k,))


def _members(t, nb):
    return [t] if nb is None else list(t.unbind(0))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nb,k", SHAPES)
@pytest.mark.parametrize("name", ["dups", "full", "blocks", "arrow129", "gaps"])
def test_matvec_matches_dense_and_autograd(name, nb, k, dt):
    tdt, npdt = DT[dt]
    c, pat = R.case(name), R.pattern(name)
    n, rows, cols, tri, nnz = c["n"], c["rows"], c["cols"], c["triangle"], len(c["rows"])
    rng = np.random.default_rng(41)
    v = rng.uniform(-1, 1, (() if nb is None else (nb,)) + (nnz,)).astype(npdt)
    x = rng.uniform(-1, 1, _shape(n, nb, k)).astype(npdt)
    w = rng.uniform(-1, 1, x.shape).astype(npdt)
    dv, dx = (torch.tensor(a, device="cuda", requires_grad=True) for a in (v, x))
    y = S.matvec(pat, dv, dx)
    assert y.shape == dx.shape and y.dtype == tdt
    (y * torch.from_numpy(w).cuda()).sum().backward()
    cv, cx = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (v, x))
    yd = torch.stack([_dense(c, a) @ b for a, b in zip(_members(cv, nb), _members(cx, nb))])
    yd = yd[0] if nb is None else yd
    (yd * torch.from_numpy(w.astype(np.float64))).sum().backward()
    got, gv, gx = y.detach().cpu().numpy(), dv.grad.cpu().numpy(), dx.grad.cpu().numpy()
    for b in range(nb or 1):
        at = (lambda a: a) if nb is None else (lambda a: a[b])
        bound = R.mv_bound(n, rows, cols, tri, at(v), at(x), npdt)
        assert np.all(np.abs(at(got) - at(yd.detach().numpy())) <= bound), ("forward", b)
        gbound = R.mv_bound(n, rows, cols, tri, at(v), at(w), npdt)
        assert np.all(np.abs(at(gx) - at(cx.grad.numpy())) <= gbound), ("grad x", b)
        obound = R.outer_bound(n, rows, cols, at(w), at(x), npdt)
        assert np.all(np.abs(at(gv) - at(cv.grad.numpy())) <= obound), ("grad values", b)
        assert not at(gv)[rows < cols].any()


def _spd_values(c, rng, lead=()):
    """values that make the matrix of case c diagonally dominant: small off-diagonal contributions, and on
    every diagonal position contributions that sum to more than its row's"""
    rows, cols, n = c["rows"], c["cols"], c["n"]
    v = rng.uniform(-0.05, 0.05, lead + (len(rows),))
    diag = rows == cols
    count = np.bincount(rows[diag], minlength=n)
    assert count.min() >= 1
    v[..., diag] = rng.uniform(4.0, 5.0, lead + (int(diag.sum()),)) / count[rows[diag]]
    return v


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("nb,k", SHAPES)
@pytest.mark.parametrize("name", ["dups", "blocks"])
def test_quad_form_and_log_prob_match_multivariate_normal(name, nb, k, dt):
    tdt, npdt = DT[dt]
    c, pat = R.case(name), R.pattern(name)
    n = c["n"]
    rng = np.random.default_rng(42)
    v = _spd_values(c, rng, () if nb is None else (nb,)).astype(npdt)
    x = rng.uniform(-1, 1, _shape(n, nb, k)).astype(npdt)
    mu = rng.uniform(-1, 1, x.shape).astype(npdt)
    out_shape = (() if nb is None else (nb,)) + (() if k is None else (k,))
    w = rng.uniform(0.5, 1.5, out_shape).astype(npdt)

    cv, cx, cm = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (v, x, mu))

    def dense():
        lps, qfs = [], []
        for a, xb, mb in zip(_members(cv, nb), _members(cx, nb), _members(cm, nb)):
            A = _dense(c, a)
            xs, ms = (xb, mb) if k is None else (xb.T, mb.T)  # [k, n]: batch of points
            lps.append(torch.distributions.MultivariateNormal(ms, precision_matrix=A).log_prob(xs))
            qfs.append(((A @ xb) * xb).sum(0))
        return tuple(torch.stack(t)[0] if nb is None else torch.stack(t) for t in (lps, qfs))

    lpd, qfd = dense()
    wd = torch.from_numpy(w.astype(np.float64))

    dv, dx, dm = (torch.tensor(a, device="cuda", requires_grad=True) for a in (v, x, mu))
    qf = S.quad_form(pat, dv, dx)
    assert qf.shape == out_shape and qf.dtype == tdt
    torch.testing.assert_close(qf.detach().cpu().double(), qfd.detach(), **TOL[dt])
    lp = S.log_prob(pat, dv, dx, dm)
    assert lp.shape == out_shape and lp.dtype == tdt
    torch.testing.assert_close(lp.detach().cpu().double(), lpd.detach(), **TOL[dt])
    (lp * torch.from_numpy(w).cuda()).sum().backward()
    (lpd * wd).sum().backward()
    for what, a, b in (("values", dv, cv), ("x", dx, cx), ("mu", dm, cm)):
        torch.testing.assert_close(a.grad.cpu().double(), b.grad, msg=lambda m: "%s: %s" % (what, m), **TOL[dt])
    # mu = None is mu = 0, and quad_form's own gradients
    lp0 = S.log_prob(pat, dv.detach(), dx.detach())
    torch.testing.assert_close(lp0, S.log_prob(pat, dv.detach(), dx.detach(), torch.zeros_like(dx)), rtol=0, atol=0)
    for t in (dv, dx, cv, cx):
        t.grad = None
    (S.quad_form(pat, dv, dx) * torch.from_numpy(w).cuda()).sum().backward()
    (dense()[1] * wd).sum().backward()
    for what, a, b in (("values", dv, cv), ("x", dx, cx)):
        torch.testing.assert_close(a.grad.cpu().double(), b.grad, msg=lambda m: "%s: %s" % (what, m), **TOL[dt])


@pytest.fixture(scope="module")
def grid_patterns():
    return {name: S.SymmetricPattern(R.refine_case(name)["rows"], R.refine_case(name)["cols"], R.refine_case(name)["n"])
            for name in R.GRIDS}


@pytest.mark.parametrize("name", list(R.GRIDS))
def test_solve_refined_reaches_the_reference(name, grid_patterns):
    c, pat = R.refine_case(name), grid_patterns[name]
    v = torch.from_numpy(c["values"]).cuda()
    b = torch.from_numpy(c["b"]).cuda()
    x = S.solve_refined(pat, v, b, iters=R.REFINE_ITERS)
    assert x.shape == b.shape and x.dtype == torch.float64
    err = R.rel_err(x.cpu().numpy(), c["ref"])
    err32 = R.rel_err(S.solve(pat, v.float(), b.float()).cpu().numpy(), c["ref"])
    print("%s: solve_refined %.3g  bound %.3g  host model %.3g  fp32 solve %.3g" % (
        name, err, R.refine_bound(name), c["model_err"], err32))
    assert err <= R.refine_bound(name)
    assert err * 1000 <= err32
    # one right-hand side [n], and a batch of two matrices: the same accuracy
    x1 = S.solve_refined(pat, v, b[:, 0].contiguous())
    assert x1.shape == (c["n"],)
    assert R.rel_err(x1.cpu().numpy(), c["ref"][:, 0]) <= R.refine_bound(name)
    xb = S.solve_refined(pat, torch.stack([v, v]), torch.stack([b, b.flip(-1)]), iters=R.REFINE_ITERS)
    assert xb.shape == (2,) + b.shape
    assert R.rel_err(xb[0].cpu().numpy(), c["ref"]) <= R.refine_bound(name)
    assert R.rel_err(xb[1].cpu().numpy(), c["ref"][:, ::-1]) <= R.refine_bound(name)


@pytest.mark.parametrize("nb,k", SHAPES)
def test_solve_refined_gradients_match_solve(nb, k, grid_patterns):
    name = "g12_s0.1"
    c, pat = R.refine_case(name), grid_patterns[name]
    n = c["n"]
    rng = np.random.default_rng(43)
    lead = () if nb is None else (nb,)
    v = c["values"] * rng.uniform(0.9, 1.1, lead + (len(c["values"]),)) * np.where(c["rows"] == c["cols"], 1.2, 1.0)
    b = rng.uniform(-1, 1, _shape(n, nb, k))
    w = torch.from_numpy(rng.uniform(-1, 1, b.shape)).cuda()
    grads = []
    for fn in (S.solve_refined, S.solve):
        dv, db = (torch.tensor(a, device="cuda", requires_grad=True) for a in (v, b))
        x = fn(pat, dv, db)
        (x * w).sum().backward()
        grads.append((x.detach(), dv.grad, db.grad))
    for what, a, e in zip(("x", "values", "b"), *grads):
        torch.testing.assert_close(a, e, msg=lambda m: "%s: %s" % (what, m), **TOL["f64"])


def test_solve_refined_stream_iters0_and_refusals(grid_patterns):
    name = "g12_s0.1"
    c, pat = R.refine_case(name), grid_patterns[name]
    v = torch.from_numpy(c["values"]).cuda().requires_grad_()
    b = torch.from_numpy(c["b"]).cuda().requires_grad_()
    w = torch.rand_like(b)

    def run():
        v.grad = b.grad = None
        x = S.solve_refined(pat, v, b)
        y = S.matvec(pat, v, x)
        ((x + y) * w).sum().backward()
        return x.detach(), v.grad.clone(), b.grad.clone()

    x0, gv0, gb0 = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x1, gv1, gb1 = run()
    torch.cuda.current_stream().wait_stream(s)
    assert pat.solver._stream is None
    for a, e in ((x1, x0), (gv1, gv0), (gb1, gb0)):
        torch.testing.assert_close(a, e, **TOL["f64"])
    # iters = 0: the fp32 solve cast up
    xz = S.solve_refined(pat, v.detach(), b.detach(), iters=0)
    assert xz.shape == b.shape and xz.dtype == torch.float64 and bool(torch.isfinite(xz).all())
    # refusals
    with pytest.raises(TypeError, match="float64"):
        S.solve_refined(pat, v.detach().float(), b.detach().float())
    with pytest.raises(TypeError, match="float64"):
        S.solve_refined(pat, v.detach(), b.detach().float())
    with pytest.raises(ValueError, match="iters"):
        S.solve_refined(pat, v.detach(), b.detach(), iters=-1)
    with pytest.raises(ValueError, match="b must be"):
        S.solve_refined(pat, v.detach(), b.detach()[:-1])
    with pytest.raises(TypeError, match="dtype"):
        S.matvec(pat, v.detach(), b.detach().float())
    with pytest.raises(ValueError, match="must be"):
        S.matvec(pat, v.detach(), b.detach()[:-1])
    with pytest.raises(ValueError, match="mu must be"):
        S.log_prob(pat, v.detach(), b.detach(), b.detach()[:, :1])
    with pytest.raises(TypeError, match="SymmetricPattern"):
        S.matvec(object(), v.detach(), b.detach())
