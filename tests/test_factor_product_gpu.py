"""GPU: the products with the factor, y = L x and y = L^T x (Solver.mulL / mulLt, bsp_factor_product_*,
DESIGN.md section 22) on the MI355X.

Parity is element-wise against factor_product_ref.py: |y_i - ref_i| <= t_i eps s_i, the bound of a length-t_i
inner product in any order (ref in longdouble for fp64 and in float64 for fp32), on random data in the layout
whose strictly-upper diagonal-block elements hold the sentinel NaN.  Operands sit in one frame between guards,
one element off the allocation's alignment, with leading dimensions above the order and different for x and y;
the output starts full of the sentinel.  Then the bitwise properties (a second run, a column alone, a batch
member alone, a Solver with a history), the identities with the half-solves and with sparse.matvec, and the
autograd layer (gradcheck, whiten undoes sample, |whiten|^2 is the quadratic form)."""
import ctypes

import numpy as np
import pytest
import torch

from baspacho_amd import autograd as BA
from baspacho_amd import sparse as S
import buffer_edges as E
import factor_product_ref as R
import helpers as H
import kf_structures as K
import sym_product_ref as SP

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
BITWISE = ["bal", "tridiag", "dense257", "width65", "chains210", "splitk513"]


def product(sol, which, L, x, ldx, y, ldy, k):
    """the C entry itself: its two leading dimensions are separate arguments"""
    fn = getattr(sol._lib, "bsp_factor_product_" + ("f64" if L.dtype == torch.float64 else "f32"))
    rc = fn(sol._h, ctypes.c_void_p(L.data_ptr()), ctypes.c_int32(which), ctypes.c_void_p(x.data_ptr()),
            ctypes.c_int64(ldx), ctypes.c_void_p(y.data_ptr()), ctypes.c_int64(ldy), ctypes.c_int32(k))
    assert rc == 0, sol._lib.bsp_last_error().decode()


def _sentinel_array(size, npdt):
    out = np.empty(size, dtype=npdt)
    out.view(np.uint64 if npdt == np.float64 else np.uint32)[:] = E.SENTINEL_BITS[npdt]
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("which", [0, 1], ids=["Lx", "Ltx"])
@pytest.mark.parametrize("name", R.structure_names())
def test_parity_in_a_hostile_frame(name, which, dt):
    tdt, npdt = DT[dt]
    sol = R.solver(name)
    n, k = sol.order(), 3
    ldx, ldy = n + 3, n + 5
    data, x = R.random_operands(sol, npdt, k, seed=17 + which)
    assert E.is_sentinel(data).sum() == len(E.upper_words(sol))
    fr = E.framed(npdt, [data, E.strided(x, ldx, npdt), _sentinel_array(k * ldy, npdt)])
    Lv, xv, yv = fr.views()
    assert Lv.data_ptr() % 16 != 0 and xv.data_ptr() % 16 != 0 and yv.data_ptr() % 16 != 0
    product(sol, which, Lv, xv, ldx, yv, ldy, k)
    torch.cuda.synchronize()
    fr.assert_intact(read_only=(0, 1), what=name)
    yh = fr.host(2)
    E.assert_padding_intact(yh, n, ldy, k, name)
    got = yh.reshape(k, ldy)[:, :n].T
    assert not E.is_sentinel(np.ascontiguousarray(got)).any(), "an element of y was not written"
    R.check(sol, data, x, got, bool(which), name)


def _dev_operands(sol, tdt, npdt, k, seed):
    data, x = R.random_operands(sol, npdt, k, seed)
    return torch.from_numpy(data).cuda(), torch.from_numpy(np.ascontiguousarray(x.T)).cuda(), data, x


def _run(sol, which, L, xt, k=None):
    """a fresh result of mulL / mulLt on [k, n] columns, the output pre-filled with the sentinel"""
    out = torch.from_numpy(_sentinel_array(xt.numel(), DT["f64" if xt.dtype == torch.float64 else "f32"][1])
                           ).cuda().reshape(xt.shape)
    got = (sol.mulLt if which else sol.mulL)(L, xt, out=out, nRHS=xt.shape[0] if k is None else k)
    assert got is out
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("which", [0, 1], ids=["Lx", "Ltx"])
@pytest.mark.parametrize("name", BITWISE)
def test_bitwise_reruns_columns_and_batches(name, which, dt):
    tdt, npdt = DT[dt]
    sol = R.solver(name)
    L, xt, data, x = _dev_operands(sol, tdt, npdt, 17, seed=23)
    full = _run(sol, which, L, xt)
    again = _run(sol, which, L, xt)
    torch.cuda.synchronize()
    assert E.bitwise_equal(full.cpu().numpy(), again.cpu().numpy()), "two runs differ"
    R.check(sol, data, x, full.cpu().numpy().T, bool(which), name)
    # column c of an nRHS = 2 and an nRHS = 17 call is the nRHS = 1 call on that column
    two = _run(sol, which, L, xt[3:5].contiguous())
    for c in range(17):
        alone = _run(sol, which, L, xt[c:c + 1].contiguous())
        assert E.bitwise_equal(alone.cpu().numpy()[0], full.cpu().numpy()[c]), ("column of 17", c)
        if c in (3, 4):
            assert E.bitwise_equal(alone.cpu().numpy()[0], two.cpu().numpy()[c - 3]), ("column of 2", c)
    # member q of a batch is the single call
    rng = np.random.default_rng(5)
    for nb in (1, 2, 5):
        Ls = [torch.from_numpy(E.poison_upper(rng.uniform(-1, 1, sol.dataSize()).astype(npdt), sol)).cuda()
              for _ in range(nb)]
        xs = [torch.from_numpy(rng.uniform(-1, 1, (2, sol.order())).astype(npdt)).cuda() for _ in range(nb)]
        outs = (sol.mulLt if which else sol.mulL)(Ls, xs, nRHS=2)
        assert isinstance(outs, list) and len(outs) == nb
        for q in range(nb):
            single = _run(sol, which, Ls[q], xs[q])
            assert E.bitwise_equal(single.cpu().numpy(), outs[q].cpu().numpy()), ("batch", nb, q)


@pytest.mark.parametrize("name", ["bal", "width65"])
def test_result_does_not_depend_on_the_solvers_history(name):
    fresh, used = R.build(name), R.build(name)
    data = H.spd_data(used, 7)
    F = torch.from_numpy(data).cuda()
    used.factor(F)
    b = torch.randn(2, used.order(), dtype=torch.float64, device="cuda")
    used.solve(F, b, nRHS=2)
    used.selectedInverse(F.clone())
    used.mulLt([F, F.clone()], [b, b.clone()], nRHS=2)
    L, xt, _, _ = _dev_operands(fresh, torch.float64, np.float64, 3, seed=29)
    for which in (1, 0):
        a, c = _run(fresh, which, L, xt), _run(used, which, L, xt)
        torch.cuda.synchronize()
        assert E.bitwise_equal(a.cpu().numpy(), c.cpu().numpy()), which


@pytest.mark.parametrize("name", ["bal", "forest", "width129"])
def test_mul_lt_undoes_solve_lt(name):
    """w = mulLt(solveLt(v)) against v.  The product step adds at most t_i eps s_i with s = |L^T| |z|, z the
    computed solution.  The solve is backward stable: (L^T + dL) z = v with |dL| <= gamma_t |L^T| for
    substitution, so |L^T z - v| <= t_i eps s_i; the solve here works by inverted diagonal blocks, which
    multiplies that by the condition number of a diagonal block, below 2 for this diagonally dominant matrix
    (diagonal 1.5 n against off-diagonal elements in [-1, 1]).  Together: 3 t_i eps s_i."""
    sol = R.solver(name)
    n, k = sol.order(), 2
    F = torch.from_numpy(H.spd_data(sol, 3)).cuda()
    sol.factor(F)
    v = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (k, n))).cuda()
    z = v.clone()
    sol.solveLt(F, z, nRHS=k)
    w = sol.mulLt(F, z, nRHS=k)
    torch.cuda.synchronize()
    Fh = F.cpu().numpy()
    _, t, s = R.reference(sol, Fh, z.cpu().numpy().T, True)
    err = np.abs(w.cpu().numpy().T - v.cpu().numpy().T)
    assert np.all(err <= 3 * R.bound(t, s, np.float64)), float((err / (R.bound(t, s, np.float64) + 1e-300)).max())


def _spd_values(c, rng, lead=()):
    """values that make the matrix of case c diagonally dominant"""
    rows, cols, n = c["rows"], c["cols"], c["n"]
    v = rng.uniform(-0.05, 0.05, lead + (len(rows),))
    diag = rows == cols
    count = np.bincount(rows[diag], minlength=n)
    v[..., diag] = rng.uniform(4.0, 5.0, lead + (int(diag.sum()),)) / count[rows[diag]]
    return v


def _factor_host(pat, v):
    """(L, |L|) dense lower factor in internal order of the pattern's matrix, from the device factor"""
    sol = pat.solver
    Ld = BA.cholesky(sol, S.assemble(pat, v)).detach().cpu().numpy()
    L = R.dense_lower(sol, Ld)
    return Ld, L, np.abs(L)


@pytest.mark.parametrize("name", ["blocks", "dups", "arrow129"])
def test_mul_l_of_mul_lt_is_the_matrix_product(name):
    """y = mulL(mulLt(x)) against A x from sparse.matvec, in internal order.  With u = fl(L^T x) and y = fl(L u):
    |y - L L^T x| <= (t_i + max_j t'_j) eps (|L| |L^T| |x|)_i, t and t' the term counts of the rows of L and of
    L^T.  The computed factor has |A - L L^T| <= gamma_{t_i + 1} |L| |L^T| (Higham, Accuracy and Stability,
    thm 10.3, with the row's term count for n), which adds (t_i + 1) eps (|L| |L^T| |x|)_i.  matvec itself is
    within sym_product_ref.mv_bound of A x."""
    c, pat = SP.case(name), SP.pattern(name)
    sol, n = pat.solver, c["n"]
    rng = np.random.default_rng(8)
    vh = _spd_values(c, rng)
    v = torch.from_numpy(vh).cuda()
    F = S.assemble(pat, v).clone()
    sol.factor(F)
    xi = torch.from_numpy(rng.uniform(-1, 1, n)).cuda()
    y = sol.mulL(F, sol.mulLt(F, xi))
    xu = pat.fromInternal(xi)
    Ax = pat.toInternal(S.matvec(pat, v, xu))
    torch.cuda.synchronize()
    L = R.dense_lower(sol, F.cpu().numpy())
    mask = R.stored_lower(sol)
    t, tt = mask.sum(1), mask.sum(0)
    llx = np.abs(L) @ (np.abs(L).T @ np.abs(xi.cpu().numpy()))
    mv = SP.mv_bound(n, c["rows"], c["cols"], c["triangle"], vh, xu.cpu().numpy(), np.float64)
    lim = (2 * t + tt.max() + 1) * np.finfo(np.float64).eps * llx + pat.toInternal(torch.from_numpy(mv).cuda()).cpu().numpy()
    err = np.abs(y.cpu().numpy() - Ax.cpu().numpy())
    assert np.all(err <= lim), float((err / lim).max())


def _grad_solvers():
    return {"random_elim": lambda: H.solver_random(71, size=8, fill=0.2, elim=(0, 4), ranges=[0, 4], pmin=1, pmax=3)[0],
            "dense11": lambda: K.dense_solver(11, span=4)}


@pytest.mark.parametrize("nb", [None, 2])
@pytest.mark.parametrize("case", list(_grad_solvers()))
def test_gradcheck_mul_l_and_mul_lt(case, nb):
    sol = _grad_solvers()[case]()
    lead = () if nb is None else (nb,)
    rng = np.random.default_rng(12)
    L = torch.tensor(rng.uniform(-1, 1, lead + (sol.dataSize(),)), device="cuda", requires_grad=True)
    x = torch.tensor(rng.uniform(-1, 1, lead + (sol.order(), 2)), device="cuda", requires_grad=True)
    x1 = torch.tensor(rng.uniform(-1, 1, lead + (sol.order(),)), device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda L_, x_: BA.mul_l(sol, L_, x_), (L, x))
    assert torch.autograd.gradcheck(lambda L_, x_: BA.mul_lt(sol, L_, x_), (L, x))
    assert torch.autograd.gradcheck(lambda L_, x_: BA.mul_lt(sol, L_, x_), (L, x1))
    # chained with cholesky: down to the matrix values
    d = torch.tensor(np.stack([H.spd_data(sol, 5 + q) for q in range(nb or 1)]).reshape(lead + (-1,)), device="cuda",
                     requires_grad=True)
    assert torch.autograd.gradcheck(lambda d_, x_: BA.mul_l(sol, BA.cholesky(sol, d_), x_), (d, x1))


@pytest.mark.parametrize("nb", [None, 2])
@pytest.mark.parametrize("name", ["blocks", "dups"])
def test_gradcheck_whiten_and_sample_cov(name, nb):
    c, pat = SP.case(name), SP.pattern(name)
    lead = () if nb is None else (nb,)
    rng = np.random.default_rng(13)
    v = torch.tensor(_spd_values(c, rng, lead), device="cuda", requires_grad=True)
    x = torch.tensor(rng.uniform(-1, 1, lead + (c["n"], 2)), device="cuda", requires_grad=True)
    mu = torch.tensor(rng.uniform(-1, 1, lead + (c["n"], 2)), device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v_, x_, m_: S.whiten(pat, v_, x_, m_), (v, x, mu))
    assert torch.autograd.gradcheck(lambda v_, z_, m_: S.sample_cov(pat, v_, z_, m_), (v, x, mu))
    assert torch.autograd.gradcheck(lambda v_, x_: S.whiten(pat, v_, x_), (v, x[..., 0].detach().requires_grad_()))


@pytest.mark.parametrize("nb,k", [(None, None), (None, 3), (2, None), (3, 2)])
@pytest.mark.parametrize("name", ["blocks", "dups"])
def test_whiten_undoes_sample_and_squares_to_the_quadratic_form(name, nb, k):
    """whiten(sample(z, mu), mu) against z at 3 t_i eps s_i, s = |L^T| |L^-T z| (the bound of
    test_mul_lt_undoes_solve_lt), plus what adding and subtracting mu costs: x = fl(mu + d) and r = fl(x - mu)
    differ from d by at most eps/2 (|x| + |r|), which the product maps to |L^T| eps/2 (|x| + |r|); eps is used
    for eps/2.  sum(whiten(x)^2) against quad_form(x - mu): with
    e_i <= t_i eps s_i the error of w_i, the sum of squares is within 2 sum |w_i| e_i + (n + 1) eps sum w_i^2 of
    |L^T r|^2; the computed factor moves that by (t_max + 1) eps |r|^T |L| |L^T| |r| from r^T A r; quad_form's own
    sums (a matvec row and a dot product) are within (t_max + n + 1) eps |r|^T |A| |r|."""
    c, pat = SP.case(name), SP.pattern(name)
    sol, n = pat.solver, c["n"]
    lead = () if nb is None else (nb,)
    tail = () if k is None else (k,)
    rng = np.random.default_rng(14)
    vh = _spd_values(c, rng, lead)
    v = torch.from_numpy(vh).cuda()
    z = torch.from_numpy(rng.uniform(-1, 1, lead + (n,) + tail)).cuda()
    mu = torch.from_numpy(rng.uniform(-1, 1, lead + (n,) + tail)).cuda()
    x = S.sample(pat, v, z, mu)
    back = S.whiten(pat, v, x, mu)
    assert back.shape == z.shape
    r = x - mu
    w = S.whiten(pat, v, r)
    cov = S.sample_cov(pat, v, z, mu)
    q = S.quad_form(pat, v, r)
    torch.cuda.synchronize()
    eps = np.finfo(np.float64).eps
    dim = len(lead)
    mask = R.stored_lower(sol)
    tt = mask.sum(0).astype(np.float64)
    zi, bi, ri, wi, ci, xi = (pat.toInternal(a, dim).cpu().numpy().reshape(lead + (n, -1))
                              for a in (z, back, r, w, cov - mu, x))
    qh = q.cpu().numpy().reshape(lead + (-1,))
    for b in range(nb or 1):
        at = (lambda a: a) if nb is None else (lambda a: a[b])
        _, L, aL = _factor_host(pat, at(v))
        s = aL.T @ np.abs(np.linalg.solve(L.T, at(zi)))
        err = np.abs(at(bi) - at(zi))
        lim = 3 * tt[:, None] * eps * s + aL.T @ (eps * (np.abs(at(xi)) + np.abs(at(ri))))
        assert np.all(err <= lim), ("whiten(sample)", b, float((err / lim).max()))
        # sample_cov: x - mu = L z at t_i eps s_i (one more eps |x| for adding and removing mu)
        tl = mask.sum(1).astype(np.float64)
        lim = tl[:, None] * eps * (aL @ np.abs(at(zi))) + 2 * eps * (np.abs(at(ci)) + np.abs(pat.toInternal(at(mu), 0).cpu().numpy().reshape(n, -1)))
        assert np.all(np.abs(at(ci) - L @ at(zi)) <= lim), ("sample_cov", b)
        # the quadratic form
        ar, aw = np.abs(at(ri)), np.abs(at(wi))
        e = tt[:, None] * eps * (aL.T @ ar)
        A = SP.abs_dense(n, c["rows"], c["cols"], at(vh))
        sp_ = sol.scalarPermutation()
        Ai = np.zeros_like(A)
        Ai[np.ix_(sp_, sp_)] = A
        lim = (2 * (aw * e).sum(0) + (n + 1) * eps * (aw ** 2).sum(0) + (tt.max() + 1) * eps * ((aL.T @ ar) ** 2).sum(0)
               + (tt.max() + n + 1) * eps * (ar * (Ai @ ar)).sum(0))
        got = (at(wi) ** 2).sum(0)
        assert np.all(np.abs(got - at(qh)) <= lim), ("quad_form", b, np.abs(got - at(qh)) / lim)
