"""GPU: the implicit Schur elimination of DESIGN.md section 29 on the MI355X.  build, mv, reduce, backSubstitute and
the reduced solve of sparse.lstsq_cg(eliminate=...) must be bitwise the numpy restatement (schur_ref.py) -- the
vectors, the state records and the status of the eliminated blocks -- in f64 and f32, with and without damping and
x0, for precond None, "jacobi", "block_jacobi" and a callable, with r alone, c alone and both, q in {1, 3}, a batch
of 2, on the bundle-adjustment like case, the narrow and
wide eliminated params, the hub case and bidiagonal kept parts whose nK crosses every chunk limit of the
reductions.  The inverses are bitwise the blocks of the full operator's block-Jacobi preconditioner; mv is the dense
S p within a bound from the term counts.  Within the GPU results: the same bits for every check_every, for a column
or a member alone and among others, for a fresh map and a used one, with framed operands; a frozen column; the stop
reasons.  Against dense float64 solves, lstsq_cg without eliminate and sparse.lstsq; gradients by gradcheck."""
import functools

import numpy as np
import pytest
import torch

from baspacho_amd import cgls as CGLS
from baspacho_amd import sparse as S
from baspacho_amd.autograd import _OnCurrentStream
from buffer_edges import framed
import cg_ref as R
import cgls_ref as C
import normal_eq_ref as N
import schur_ref as SR

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
AB = SR.DENSE_DAMPING
PIECES = ["ba", "w1", "w8", "hub", "bidiag_1", "bidiag_255", "bidiag_256", "bidiag_1024", "bidiag_1025"]


def _dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _kept_jacobi(mdl):
    """a callable preconditioner on the kept scalars, as (numpy, torch factory): z = s / (colsq + d)"""
    ks = mdl.t["kept_scalar"]
    den = mdl.csq[ks] + (0.0 if mdl.d is None else mdl.d[ks].astype(np.float64))
    inv = (1.0 / den).astype(mdl.dt)
    return (lambda s: (s * inv[:, None]).astype(mdl.dt)), inv


def _solve(sch, v, r=None, c=None, ab=None, precond=None, tol=1e-10, max_steps=12, check_every=8, x0=None):
    """the run lstsq_cg(eliminate=...) makes (c None) or its backward pass makes (r None): (x, info)"""
    cache = {}
    with _OnCurrentStream(sch.jop.solver, v.device):
        x, run = S._schur_run(sch, v, r, c, ab, precond, tol, max_steps, check_every, x0, cache)
    info = {"iterations": run.iterations(), "stop": run.stop(), "state": run.state,
            "eliminate_status": cache["eliminate_status"], "binv": cache["binv"]}
    if isinstance(precond, str):
        info["precond_status"] = cache[precond].status
    return x, info


def _check(got_x, info, want_x, st, status, what, pstatus=None):
    assert _bits(got_x) == _bits(want_x), (what, "x", np.abs(got_x.cpu().numpy() - want_x).max())
    state = info["state"].cpu().numpy().reshape(-1, 12)
    for j in range(state.shape[0]):
        np.testing.assert_array_equal(state[j], R.record_words(st, j), err_msg="%s column %d" % (what, j))
    np.testing.assert_array_equal(info["eliminate_status"].cpu().numpy(), status, err_msg=str(what))
    if pstatus is not None:
        np.testing.assert_array_equal(info["precond_status"].cpu().numpy(), pstatus, err_msg=str(what))


@functools.lru_cache(maxsize=None)
def _vectors(name, npdt, q):
    c, _ = SR.case(name)
    rng = np.random.default_rng(q + c["m"])
    return rng.uniform(-1, 1, (c["m"], q)).astype(npdt), rng.uniform(-1, 1, (c["n"], q)).astype(npdt)


# ---- the pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", PIECES)
def test_pieces_bitwise_against_the_restatement(name, dt):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator(name)
    v = _dev(c["values"], tdt)
    for damped in (False, True):
        mdl = SR.model(name, npdt, damped)
        with _OnCurrentStream(jop.solver, v.device):
            d = None if not damped else CGLS.damping_vector(jop.product, CGLS.column_norms(jop.product, v), AB[0], AB[1], v)
            binv, status = sch.map.build(v, d)
            assert _bits(binv[:len(mdl.binv)]) == _bits(mdl.binv), (name, dt, damped, "binv")
            np.testing.assert_array_equal(status.cpu().numpy(), mdl.status)
            for q in (1, 3):
                _, g = _vectors(name, npdt, q)
                p = g[mdl.t["kept_scalar"]]
                t = torch.full((c["m"], q), float("nan"), dtype=tdt, device="cuda")
                out = sch.map.mv(v, binv, _dev(p, tdt), d=d, t=t)
                want, want_t = mdl.mv_t(p)
                assert _bits(out) == _bits(want) and _bits(t) == _bits(want_t), (name, dt, damped, q, "mv")
                bk = sch.map.reduce(v, binv, _dev(g, tdt))
                assert _bits(bk) == _bits(mdl.reduce(g)), (name, dt, damped, q, "reduce")
                x = sch.map.backSubstitute(v, binv, _dev(g, tdt), _dev(p, tdt))
                assert _bits(x) == _bits(mdl.back(g, p)), (name, dt, damped, q, "back")
            # [rows] operands are the [rows, 1] ones
            _, g = _vectors(name, npdt, 1)
            p = _dev(g[mdl.t["kept_scalar"], 0], tdt)
            assert _bits(sch.map.mv(v, binv, p, d=d)) == _bits(mdl.mv(g[mdl.t["kept_scalar"]]))
            assert sch.map.reduce(v, binv, _dev(g[:, 0], tdt)).shape == (mdl.nK,)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["ba", "hub"])
def test_a_batch_of_two_is_its_members(name, dt):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator(name)
    vals = np.stack([c["values"], 0.9 * c["values"]]).astype(npdt)
    _, g = _vectors(name, npdt, 3)
    gg = np.stack([g, -0.5 * g]).astype(npdt)
    v = _dev(vals, tdt)
    with _OnCurrentStream(jop.solver, v.device):
        d = CGLS.damping_vector(jop.product, CGLS.column_norms(jop.product, v), AB[0], AB[1], v)
        binv, status = sch.map.build(v, d)
        pk = _dev(gg[:, SR.model(name, npdt, True).t["kept_scalar"]], tdt)
        out, bk = sch.map.mv(v, binv, pk, d=d), sch.map.reduce(v, binv, _dev(gg, tdt))
        x = sch.map.backSubstitute(v, binv, _dev(gg, tdt), pk)
        for b in range(2):
            mdl = SR.Model(c, elim, npdt, values=vals[b], damping_ab=AB, t=SR.model(name, npdt, True).t)
            p = gg[b][mdl.t["kept_scalar"]]
            assert _bits(binv[b, :len(mdl.binv)]) == _bits(mdl.binv) and status[b].tolist() == mdl.status.tolist()
            assert _bits(out[b]) == _bits(mdl.mv(p)) and _bits(bk[b]) == _bits(mdl.reduce(gg[b]))
            assert _bits(x[b]) == _bits(mdl.back(gg[b], p))
            # a member alone is the member of the batch
            b1, s1 = sch.map.build(v[b], d[b])
            assert _bits(b1) == _bits(binv[b]) and _bits(s1) == _bits(status[b])
            assert _bits(sch.map.mv(v[b], b1, pk[b], d=d[b])) == _bits(out[b])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["ba", "w1", "w8", "hub"])
def test_the_inverses_are_the_blocks_of_block_jacobi(name, dt):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator(name)
    v = _dev(c["values"], tdt)
    sizes = np.asarray(c["param_sizes"], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes * sizes)])
    for damped in (False, True):
        with _OnCurrentStream(jop.solver, v.device):
            csq = CGLS.column_norms(jop.product, v)
            d = CGLS.damping_vector(jop.product, csq, AB[0], AB[1], v) if damped else None
            full = CGLS.Preconditioner(jop.product, "block_jacobi", v, csq, d).values.cpu().numpy()
            binv = sch.map.build(v, d)[0].cpu().numpy()
        want = np.concatenate([full[off[p]:off[p + 1]] for p in sorted(elim)])
        assert _bits(binv[:len(want)]) == _bits(want), (name, dt, damped)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["ba", "w8", "hub"])
def test_mv_is_the_dense_product_within_the_term_count_bound(name, dt):
    """out = J_k^T ((I - J_e Binv J_e^T) (J_k p)) + D_k p is evaluated as a chain of ordered sums: a (at most ra terms
    per row), u (cu terms per eliminated scalar), y (w terms), f (re terms), t = a - f (one rounding), the column
    sums (ck terms) and the damping (a product and an addition).  Every path from a p_c to an out_c' passes through
    at most k = ra + cu + w + re + 1 + ck + 2 roundings, each a factor (1 + delta), |delta| <= eps, on a quantity
    bounded by the product of the absolute values along the path, so (Higham, Accuracy and Stability, Lemma 3.1)
        |out - S~ p| <= gamma_k (|J_k|^T (I + |J_e| |Binv| |J_e|^T) |J_k| + D_k) |p|,  gamma_k = k eps / (1 - k eps),
    elementwise, with S~ built from the inverses the device computed (the build's own error is not the product's)."""
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator(name)
    mdl = SR.model(name, npdt, True)
    v = _dev(c["values"], tdt)
    _, g = _vectors(name, npdt, 3)
    p = g[mdl.t["kept_scalar"]]
    with _OnCurrentStream(jop.solver, v.device):
        d = CGLS.damping_vector(jop.product, CGLS.column_norms(jop.product, v), AB[0], AB[1], v)
        binv, _ = sch.map.build(v, d)
        out = sch.map.mv(v, binv, _dev(p, tdt), d=d).cpu().numpy()
    L = np.longdouble
    J = N.dense_j(c["m"], c["n"], c["rows"], c["cols"], c["values"].astype(npdt)).astype(L)
    ks, es = mdl.t["kept_scalar"], mdl.t["elim_scalar"]
    Jk, Je = J[:, ks], J[:, es]
    Bi = np.zeros((len(es), len(es)), dtype=L)
    bh = binv.cpu().numpy()
    for e, w in enumerate(mdl.t["block_width"]):
        l0 = mdl.t["elim_off"][e]
        Bi[l0:l0 + w, l0:l0 + w] = bh[mdl.block_off[e]:mdl.block_off[e + 1]].reshape(w, w)
    dk = d.cpu().numpy().astype(L)[ks]
    a = Jk @ p.astype(L)
    exact = Jk.T @ (a - Je @ (Bi @ (Je.T @ a))) + dk[:, None] * p.astype(L)
    absm = np.abs(Jk).T @ (np.abs(Jk) @ np.abs(p).astype(L) + np.abs(Je) @ (np.abs(Bi) @ (np.abs(Je).T @ (np.abs(Jk) @ np.abs(p).astype(L)))))
    absm = absm + dk[:, None] * np.abs(p).astype(L)
    longest = lambda key: int(np.diff(mdl.t[key][0]).max())
    k = longest("rows_kept") + longest("cols_elim") + int(mdl.t["block_width"].max()) + longest("rows_elim") + 1 + \
        longest("cols_kept") + 2
    eps = L(np.finfo(npdt).eps) / 2
    bound = k * eps / (1 - k * eps) * absm
    err = np.abs(out.astype(L) - exact)
    print("%s %s: k = %d, largest error / bound %.3f" % (name, dt, k, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())


# ---- the reduced solve ----------------------------------------------------------------------------------------
SOLVES = ["ba", "w1", "w8", "hub", "bidiag_1", "bidiag_255", "bidiag_256", "bidiag_1024", "bidiag_1025"]


@pytest.mark.parametrize("precond", [None, "callable", "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", SOLVES)
def test_solve_bitwise_against_the_restatement(name, dt, precond):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator(name)
    v = _dev(c["values"], tdt)
    r, cv = _vectors(name, npdt, 2)
    for damped in ((True,) if name == "hub" else (False, True)):  # (the hub case is singular without damping)
        mdl = SR.model(name, npdt, damped)
        ab = AB if damped else None
        pm, inv = _kept_jacobi(mdl) if precond == "callable" else (precond, None)
        invd = None if inv is None else _dev(inv, tdt)
        pd = (lambda s: s * invd[..., None]) if precond == "callable" else precond
        for which, kw in (("r", dict(r=r)), ("c", dict(c=cv)), ("rc", dict(r=r, c=cv)), ("x0", dict(r=r, x0=cv))):
            want, st = mdl.solve(precond=pm, max_steps=10, **kw)
            ps = mdl.precond_status if isinstance(precond, str) and precond != "callable" else None
            got, info = _solve(sch, v, ab=ab, precond=pd, max_steps=10, **{k: _dev(a, tdt) for k, a in kw.items()})
            _check(got, info, want, st, mdl.status, (name, dt, precond, damped, which), ps)
    # the public entry gives the same bits and the same records (the last run: r and x0, damped)
    x, info = S.lstsq_cg(jop, v, _dev(r, tdt), damping=AB, precond=pd, max_steps=10, x0=_dev(cv, tdt), return_info=True,
                         eliminate=sch)
    _check(x, info, want, st, mdl.status, (name, dt, precond, "lstsq_cg"), ps)
    assert ("precond_status" in info) == (ps is not None)


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_same_bits_for_every_check_every_column_and_member(dt, precond):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator("ba")
    rng = np.random.default_rng(11)
    vals = np.stack([c["values"] * s for s in (1.0, 0.7, 1.3)]).astype(npdt)
    r = rng.uniform(-1, 1, (3, c["m"], 3)).astype(npdt)
    r[1, :, 2] = 0.0
    v, rd = _dev(vals, tdt), _dev(r, tdt)
    kw = dict(damping=AB, precond=precond, tol=1e-6 if dt == "f64" else 1e-3, max_steps=40, return_info=True,
              eliminate=sch)
    x, info = S.lstsq_cg(jop, v, rd, check_every=8, **kw)
    assert info["stop"][1, 2] == 5 and (info["stop"][0] == 1).all() and not x[1, :, 2].any()
    for ce in (1, 3, None):
        x2, i2 = S.lstsq_cg(jop, v, rd, check_every=ce, **kw)
        assert _bits(x2) == _bits(x) and _bits(i2["state"]) == _bits(info["state"]), ce
    for b in range(3):
        xb, ib = S.lstsq_cg(jop, v[b], rd[b], **kw)
        assert _bits(xb) == _bits(x[b]) and _bits(ib["state"]) == _bits(info["state"][b]), b
        assert _bits(ib["eliminate_status"]) == _bits(info["eliminate_status"][b])
        for j in range(3):
            xj, ij = S.lstsq_cg(jop, v[b], rd[b, :, j].contiguous(), **kw)
            assert _bits(xj) == _bits(x[b, :, j]) and _bits(ij["state"]) == _bits(info["state"][b, j]), (b, j)
    mdl = SR.Model(c, elim, npdt, values=vals[2], damping_ab=AB)
    want, st = mdl.solve(r=r[2], precond=precond, tol=kw["tol"], max_steps=40)
    _check(x[2], {"state": info["state"][2], "eliminate_status": info["eliminate_status"][2]}, want, st, mdl.status, "member 2")


def test_frozen_column():
    # column 0 starts at the solution and stops converged at once; column 1 runs on beside it
    c, elim, jop, sch = SR.operator("ba")
    mdl = SR.model("ba", np.float64, True)
    rng = np.random.default_rng(4)
    r = rng.uniform(-1, 1, (c["m"], 2))
    xd, _ = C.dense_solution(c, r=r, damping_ab=AB)
    x0 = np.stack([xd[:, 0], rng.uniform(-1, 1, c["n"])], axis=1)
    tdt = torch.float64
    x, info = S.lstsq_cg(jop, _dev(c["values"], tdt), _dev(r, tdt), damping=AB, precond=None, tol=1e-8, max_steps=50,
                         x0=_dev(x0, tdt), return_info=True, eliminate=sch)
    assert info["stop"].tolist() == [1, 1] and info["iterations"][0] == 0 and info["iterations"][1] > 3
    ks = mdl.t["kept_scalar"]
    assert _bits(x[ks, 0]) == _bits(x0[ks, 0])  # the kept part is the start's, bit for bit
    want, st = mdl.solve(r=r, tol=1e-8, max_steps=50, x0=x0)
    _check(x, info, want, st, mdl.status, "frozen")


@pytest.mark.parametrize("case", ["zero", "breakdown", "nan", "bad_block"])
def test_stops_and_status_on_the_device(case):
    tdt = torch.float64
    if case == "zero":
        # one row (2 on the eliminated scalar 0, 1 on the kept scalar 1): B = 4, F = 2, everything exact in binary.
        # g = (4, 2): y = 1, b_k = 2 - 1 * 2 = 0: stop 5 with x_k = 0, and x_e = B^-1 g_e = 1 is still returned
        jop = S.JacobianOperator([0, 0], [0, 1], 1, 2)
        v = _dev(np.array([2.0, 1.0]), tdt)
        with _OnCurrentStream(jop.solver, v.device):
            x, run = S._schur_run(S.JacobianSchur(jop, [0]), v, None, _dev(np.array([4.0, 2.0]), tdt), None, None, 1e-10, 5,
                                  8, None, {})
        assert run.stop().tolist() == [5] and x.tolist() == [1.0, 0.0]
        x, info = S.lstsq_cg(jop, v, _dev(np.zeros(1), tdt), precond=None, eliminate=[0], return_info=True)
        assert info["stop"] == 5 and not x.any() and info["relres"] == 0 and info["eliminate_status"].tolist() == [-1, 0]
        return
    c, elim, jop, sch = SR.operator("ba")
    vals = c["values"].copy()
    mdl0 = SR.model("ba", np.float64, False)
    rng = np.random.default_rng(2)
    if case == "breakdown":
        # an all-zero kept column without damping: S is singular along e_col, the curvature of that direction is 0
        col = int(mdl0.t["kept_scalar"][5])
        vals[c["cols"] == col] = 0.0
        cv = np.zeros((c["n"], 2))
        cv[col, 0] = 1.0
        cv[:, 1] = rng.uniform(-1, 1, c["n"])
        mdl = SR.Model(c, elim, np.float64, values=vals, t=mdl0.t)
        want, st = mdl.solve(c=cv, max_steps=30)
        x, info = _solve(sch, _dev(vals, tdt), c=_dev(cv, tdt), max_steps=30)
        assert info["stop"][0] == 3 and info["iterations"][0] == 0 and st["pAp"][0] == 0.0
        _check(x, info, want, st, mdl.status, case)
    elif case == "nan":
        vals[int(np.nonzero(np.isin(c["cols"], mdl0.t["kept_scalar"]))[0][0])] = np.nan
        r = rng.uniform(-1, 1, (c["m"], 2))
        x, info = S.lstsq_cg(jop, _dev(vals, tdt), _dev(r, tdt), precond=None, eliminate=sch, return_info=True)
        assert info["stop"].tolist() == [4, 4] and info["iterations"].tolist() == [0, 0]
    else:
        # the hub case's last eliminated param has no rows: without damping its block is zero, a bad pivot
        c, elim, jop, sch = SR.operator("hub")
        mdl = SR.model("hub", np.float64, False)
        r = rng.uniform(-1, 1, (c["m"], 2))
        x, info = S.lstsq_cg(jop, _dev(c["values"], tdt), _dev(r, tdt), precond=None, max_steps=4, eliminate=sch,
                             return_info=True)
        assert info["eliminate_status"].tolist() == [int(mdl.t["elim_scalar"][-1]), 1] == mdl.status.tolist()
        assert not x[int(mdl.t["elim_scalar"][-1])].any()  # a zero inverse: the scalar stays 0
        want, st = mdl.solve(r=r, max_steps=4)
        _check(x, info, want, st, mdl.status, case)


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", SR.DENSE_CASES)
def test_against_dense_float64_lstsq_cg_and_lstsq(name, dt, precond):
    """the CPU test's bound: kappa(N) tol on the relative error of the full x, kappa(N) <= 100 from the dense matrix"""
    tdt, npdt = DT[dt]
    tol = 1e-12 if dt == "f64" else 1e-6
    c, elim, jop, sch = SR.operator(name)
    r = np.random.default_rng(5).uniform(-1, 1, (c["m"], 2)).astype(npdt)
    xd, Nm = C.dense_solution(c, r=r, damping_ab=AB, values=c["values"].astype(npdt))
    kappa = np.linalg.cond(Nm)
    assert kappa <= 100
    bound = kappa * tol
    v, rd = _dev(c["values"], tdt), _dev(r, tdt)
    x, info = S.lstsq_cg(jop, v, rd, damping=AB, precond=precond, tol=tol, max_steps=200, return_info=True, eliminate=sch)
    assert (info["stop"] == 1).all(), info["stop"]
    rel = lambda a, b: np.linalg.norm(a - b, axis=0) / np.linalg.norm(b, axis=0)
    err = rel(x.cpu().numpy().astype(np.float64), xd)
    plain, pinfo = S.lstsq_cg(jop, v, rd, damping=AB, precond=precond, tol=tol, max_steps=200, return_info=True)
    pat = S.JacobianPattern(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
    xl = S.lstsq(pat, v, rd, damping=AB)
    d1 = rel(x.cpu().numpy().astype(np.float64), plain.cpu().numpy().astype(np.float64))
    d2 = rel(x.cpu().numpy().astype(np.float64), xl.cpu().numpy().astype(np.float64))
    print("%s %s %s: kappa %.1f, iterations %s (plain %s), error against dense %s, lstsq_cg %s, lstsq %s, bound %.1e" % (
        name, dt, precond, kappa, info["iterations"].tolist(), pinfo["iterations"].tolist(), err, d1, d2, bound))
    assert (err <= bound).all() and (d1 <= bound).all() and (d2 <= bound).all(), (err, d1, d2, bound)
    # the index array builds the map once and keeps it on the operator
    x2 = S.lstsq_cg(jop, v, rd, damping=AB, precond=precond, tol=tol, max_steps=200, eliminate=np.asarray(elim))
    assert _bits(x2) == _bits(x) and len(jop._schur) == 1
    S.lstsq_cg(jop, v, rd, damping=AB, precond=precond, tol=tol, max_steps=200, eliminate=np.asarray(elim))
    assert len(jop._schur) == 1


def test_gradients():
    c, elim, jop, sch = SR.operator("tiny")
    assert c["n"] <= 12
    rng = np.random.default_rng(8)
    v = _dev(c["values"], torch.float64).requires_grad_()
    r = _dev(rng.uniform(-1, 1, (c["m"], 2)), torch.float64).requires_grad_()
    alpha = torch.tensor(0.3, dtype=torch.float64, device="cuda", requires_grad=True)
    beta = torch.tensor(0.2, dtype=torch.float64, device="cuda", requires_grad=True)
    for precond in (None, "block_jacobi"):
        f = lambda v, r, alpha, beta: S.lstsq_cg(jop, v, r, damping=(alpha, beta), precond=precond, tol=1e-13,
                                                 max_steps=200, eliminate=sch)
        assert torch.autograd.gradcheck(f, (v, r, alpha, beta), eps=1e-6, atol=1e-7, rtol=1e-6)
    # a batch, a single right-hand side, no damping
    vb = torch.stack([v.detach(), 1.1 * v.detach()]).requires_grad_()
    rb = torch.stack([r.detach()[:, 0], r.detach()[:, 1]]).requires_grad_()
    f = lambda v, r: S.lstsq_cg(jop, v, r, precond="jacobi", tol=1e-13, max_steps=200, eliminate=sch)
    assert torch.autograd.gradcheck(f, (vb, rb), eps=1e-6, atol=1e-7, rtol=1e-6)
    # the gradients are those of the plain solve
    g1 = torch.autograd.grad(S.lstsq_cg(jop, v, r, damping=(alpha, beta), precond=None, tol=1e-13, max_steps=200,
                                        eliminate=sch).square().sum(), (v, r, alpha, beta))
    g2 = torch.autograd.grad(S.lstsq_cg(jop, v, r, damping=(alpha, beta), precond=None, tol=1e-13, max_steps=200)
                             .square().sum(), (v, r, alpha, beta))
    for a, b in zip(g1, g2):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_framed_and_offset_operands(dt):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = SR.operator("hub")
    r, x0 = _vectors("hub", npdt, 3)
    vals = np.stack([c["values"], 0.9 * c["values"]]).astype(npdt)
    rr, xx = np.stack([r, 0.5 * r]), np.stack([x0, -x0])
    kw = dict(damping=AB, precond=None, max_steps=8, return_info=True, eliminate=sch)
    plain = S.lstsq_cg(jop, _dev(vals, tdt), _dev(rr, tdt), x0=_dev(xx, tdt), **kw)
    # every operand inside its own guards, at an odd element offset: element-aligned, never 16-byte-aligned
    fr = framed(npdt, [vals, rr, xx])
    fv, frr, fx = (fr.view(k).reshape(a.shape) for k, a in enumerate((vals, rr, xx)))
    assert all(t.data_ptr() % 16 != 0 for t in (fv, frr, fx))
    x, info = S.lstsq_cg(jop, fv, frr, x0=fx, **kw)
    fr.assert_intact(read_only=(0, 1, 2), what="lstsq_cg")
    assert _bits(x) == _bits(plain[0]) and _bits(info["state"]) == _bits(plain[1]["state"])
    # the pieces with every vector of theirs framed: the outputs stay inside their payloads
    mdl = SR.model("hub", npdt, True)
    with _OnCurrentStream(jop.solver, fv.device):
        d = CGLS.damping_vector(jop.product, CGLS.column_norms(jop.product, fv), AB[0], AB[1], fv)
        binv, _ = sch.map.build(fv, d)
        pk = xx[:, mdl.t["kept_scalar"]]
        f2 = framed(npdt, [d.cpu().numpy(), binv.cpu().numpy(), pk, xx])
        gd, gb, gp, gg = (f2.view(k).reshape(s) for k, s in enumerate((d.shape, binv.shape, pk.shape, xx.shape)))
        shapes = [(2, mdl.m, 3), (2, mdl.nK, 3), (2, mdl.nK, 3), (2, mdl.n, 3)]
        f3 = framed(npdt, [np.zeros(s, dtype=npdt) for s in shapes])
        t, out, bk, xo = (f3.view(k).reshape(s) for k, s in enumerate(shapes))
        sch.map.mv(fv, gb, gp, d=gd, out=out, t=t)
        sch.map.reduce(fv, gb, gg, out=bk, t=t)
        sch.map.backSubstitute(fv, gb, gg, gp, out=xo, t=t)
        want = (sch.map.mv(fv, binv, _dev(pk, tdt), d=d), sch.map.reduce(fv, binv, _dev(xx, tdt)),
                sch.map.backSubstitute(fv, binv, _dev(xx, tdt), _dev(pk, tdt)))
    torch.cuda.synchronize()
    f2.assert_intact(read_only=(0, 1, 2, 3), what="schur pieces")
    f3.assert_intact(what="schur pieces")
    for a, b in zip((out, bk, xo), want):
        assert _bits(a) == _bits(b)


def test_a_veteran_map_gives_the_bits_of_a_fresh_one():
    c, elim = SR.case("hub")
    jop = SR.operator("hub")[2]
    make = lambda: S.JacobianSchur(jop, np.asarray(elim))
    rng = np.random.default_rng(12)
    r = rng.uniform(-1, 1, (c["m"], 2))

    def probe(sch):
        out = []
        for dt, ab, precond in (("f64", AB, "block_jacobi"), ("f32", AB, "jacobi"), ("f64", (0.0, 0.5), None)):
            tdt = DT[dt][0]
            x, info = S.lstsq_cg(jop, _dev(c["values"], tdt), _dev(r, tdt), damping=ab, precond=precond, max_steps=6,
                                 return_info=True, eliminate=sch)
            out.append(_bits(x) + _bits(info["state"]) + _bits(info["eliminate_status"]) +
                       _bits(info.get("precond_status", torch.zeros(0))))
        return out

    veteran = make()
    for dt, nb, q in (("f32", 3, 1), ("f64", 1, 4), ("f32", 2, 2)):
        tdt = DT[dt][0]
        vals = _dev(np.stack([c["values"] * (1 + 0.1 * b) for b in range(nb)]), tdt)
        rb = _dev(rng.uniform(-1, 1, (nb, c["m"], q)), tdt)
        for precond in ("jacobi", None, "block_jacobi"):
            S.lstsq_cg(jop, vals, rb, damping=AB, precond=precond, max_steps=5, check_every=None, eliminate=veteran)
    assert probe(veteran) == probe(make())


def test_refusals():
    c, elim, jop, sch = SR.operator("w1")
    tdt = torch.float64
    v, r = _dev(c["values"], tdt), _dev(np.ones(c["m"]), tdt)
    wide = S.JacobianOperator([0, 1], [0, 40], 2, 42, param_sizes=[8, 33, 1])
    ones = _dev(np.ones(2), tdt)
    with pytest.raises(ValueError, match="param 1 has 33 scalars; 'block_jacobi' takes params of at most 32"):
        S.lstsq_cg(wide, ones, ones, eliminate=[0])
    assert S.lstsq_cg(wide, ones, ones, precond="jacobi", eliminate=[0]).shape == (42,)
    # an eliminated param may be wider than a block of block_jacobi could be ... but not wider than 8
    with pytest.raises(RuntimeError, match="eliminated param 1 has 33 scalars"):
        S.lstsq_cg(wide, ones, ones, eliminate=[1])
    other = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
    with pytest.raises(ValueError, match="eliminate was built on another operator"):
        S.lstsq_cg(other, v, r, precond=None, eliminate=sch)
    with pytest.raises(RuntimeError, match=r"jacobian schur: eliminate\[0\] = 99 is out of range"):
        S.lstsq_cg(jop, v, r, precond=None, eliminate=[99])
    with pytest.raises(ValueError, match=r"must return a tensor of shape \(%d,\)" % sch.nK):
        S.lstsq_cg(jop, v, r, precond=lambda s: s[:-1], eliminate=sch)
    with _OnCurrentStream(jop.solver, v.device):
        binv, _ = sch.map.build(v)
        with pytest.raises(ValueError, match=r"values must be \[%d\] or \[B, %d\]" % (jop.nnz, jop.nnz)):
            sch.map.build(v[:-1])
        with pytest.raises(ValueError, match="binv must be what build\\(\\) returned"):
            sch.map.mv(v, binv[:-1], torch.zeros(sch.nK, dtype=tdt, device="cuda"))
        with pytest.raises(ValueError, match=r"p must be \[%d\] or \[%d, q\]" % (sch.nK, sch.nK)):
            sch.map.mv(v, binv, torch.zeros(sch.nK + 1, dtype=tdt, device="cuda"))
        with pytest.raises(TypeError, match="g must be a torch.float64 tensor"):
            sch.map.reduce(v, binv, torch.zeros(jop.n, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError, match="the vectors must have one shape"):
            sch.map.backSubstitute(v, binv, torch.zeros(jop.n, 2, dtype=tdt, device="cuda"),
                                   torch.zeros(sch.nK, dtype=tdt, device="cuda"))
        with pytest.raises(ValueError, match="state must be the int64 records"):
            sch.map.mv(v, binv, torch.zeros(sch.nK, dtype=tdt, device="cuda"), state=torch.zeros(2, 12, dtype=torch.int64,
                                                                                                 device="cuda"))
    # without eliminate nothing changes: the trailing keyword's default is the plain path
    x1 = S.lstsq_cg(jop, v, r, precond="jacobi")
    x2 = S.lstsq_cg(jop, v, r, precond="jacobi", eliminate=None)
    assert _bits(x1) == _bits(x2)
