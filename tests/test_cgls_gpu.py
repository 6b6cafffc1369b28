"""GPU: the matrix-free least squares of DESIGN.md section 28 on the MI355X.  sparse.lstsq_cg (and the run with c
alone that its backward pass makes) must be bitwise the numpy restatement (cgls_ref.py) -- x, the state records
and the preconditioner's status -- for precond None, "jacobi" and "block_jacobi", with and without damping and x0,
in f64 and f32, on the Jacobians of normal_eq_ref, the hub case and bidiagonal Jacobians whose m and n cross every
boundary of the reductions.  The products through a JacobianOperator are bitwise ref_j_vec / ref_jt_vec.  Within
the GPU results: the same bits for every check_every, for a column or a batch member alone and among others, for
a fresh operator and a used one, with framed operands; a converged column frozen while its neighbour runs on; the
stop reasons.  Against dense float64 solves and sparse.lstsq within kappa * tol; gradients by gradcheck."""
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

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
AB = (0.25, 0.05)


def _dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _solve(op, v, r=None, c=None, ab=None, precond=None, tol=1e-10, max_steps=12, check_every=8, x0=None):
    """the run lstsq_cg makes (c None) or its backward pass makes (r None): (x, info)"""
    cache = {}
    with _OnCurrentStream(op.solver, v.device):
        x, run = S._cgls_run(op, v, r, c, ab, precond, tol, max_steps, check_every, x0, cache)
    info = {"iterations": run.iterations(), "stop": run.stop(), "state": run.state}
    if isinstance(precond, str):
        info["precond_status"] = cache[precond].status
    return x, info


def _check(got_x, info, want_x, st, status, what, j_of=lambda j: j):
    assert _bits(got_x) == _bits(want_x), (what, "x", np.abs(got_x.cpu().numpy() - want_x).max())
    state = info["state"].cpu().numpy().reshape(-1, 12)
    for j in range(state.shape[0]):
        np.testing.assert_array_equal(state[j], R.record_words(st, j_of(j)), err_msg="%s column %d" % (what, j))
    if status is not None:
        np.testing.assert_array_equal(info["precond_status"].cpu().numpy(), status, err_msg=what)


def _operands(name, npdt, q=2, seed=0):
    c, op = C.operator(name)
    rng = np.random.default_rng(seed + c["m"])
    return c, op, rng.uniform(-1, 1, (c["m"], q)).astype(npdt), rng.uniform(-1, 1, (c["n"], q)).astype(npdt)


BITWISE = ["scalar", "blocks", "blocks_elim", "hub", "empty_rows", "one", "longrun", "tiles3", "bidiag_1_1",
           "bidiag_255_255", "bidiag_256_255", "bidiag_1024_1024", "bidiag_1025_1024", "bidiag_2049_2049",
           "bidiag_2049_1025", "bidiag_1025_2049", "bidiag_255_256", "bidiag_1_255"]


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", BITWISE)
def test_bitwise_against_the_restatement(name, dt, precond):
    tdt, npdt = DT[dt]
    c, op, r, x0 = _operands(name, npdt)
    if precond == "block_jacobi" and name == "tiles3":
        with pytest.raises(ValueError, match="param 0 has 72 scalars; 'block_jacobi' takes params of at most 32"):
            S.lstsq_cg(op, _dev(c["values"], tdt), _dev(r, tdt))
        return
    v = _dev(c["values"], tdt)
    for ab in (None, AB):
        for start in (None, x0):
            what = (name, dt, precond, ab, start is not None)
            want, st, status = C.cgls_model(c, npdt, r=r, damping_ab=ab, precond=precond, max_steps=12, x0=start)
            got, info = _solve(op, v, r=_dev(r, tdt), ab=ab, precond=precond, x0=None if start is None else _dev(start, tdt))
            _check(got, info, want, st, status, what)
    # the public entry gives the same bits and the same records
    x, info = S.lstsq_cg(op, v, _dev(r, tdt), damping=AB, precond=precond, max_steps=12, x0=_dev(x0, tdt),
                         return_info=True)
    _check(x, info, want, st, status, (name, dt, precond, "lstsq_cg"))
    assert torch.equal(info["relres"], torch.sqrt(info["state"].view(torch.float64)[..., 4] /
                                                  info["state"].view(torch.float64)[..., 5]))


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["blocks", "hub", "bidiag_1025_1024"])
def test_bitwise_with_c_alone_and_with_both(name, dt, precond):
    tdt, npdt = DT[dt]
    c, op, r, cv = _operands(name, npdt, seed=3)
    v = _dev(c["values"], tdt)
    for ab in (None, AB):
        want, st, status = C.cgls_model(c, npdt, c=cv, damping_ab=ab, precond=precond, max_steps=10)
        got, info = _solve(op, v, c=_dev(cv, tdt), ab=ab, precond=precond, max_steps=10)
        _check(got, info, want, st, status, (name, dt, precond, ab, "c alone"))
    want, st, status = C.cgls_model(c, npdt, r=r, c=cv, damping_ab=AB, precond=precond, max_steps=10, x0=cv)
    got, info = _solve(op, v, r=_dev(r, tdt), c=_dev(cv, tdt), ab=AB, precond=precond, max_steps=10, x0=_dev(cv, tdt))
    _check(got, info, want, st, status, (name, dt, precond, "r and c"))


def test_more_than_256_first_pass_partials():
    # n = 256 * 1024 + 1: 257 partials of s.s and s.z, 514 of the curvature, at q = 1
    n = 256 * 1024 + 1
    name = "bidiag_%d_%d" % (n + 1, n)
    c, op, r, _ = _operands(name, np.float64, q=1)
    want, st, status = C.cgls_model(c, np.float64, r=r, damping_ab=AB, precond="jacobi", max_steps=3)
    got, info = _solve(op, _dev(c["values"], torch.float64), r=_dev(r, torch.float64), ab=AB, precond="jacobi", max_steps=3)
    _check(got, info, want, st, status, name)
    del C._OPERATORS[name]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, 3])
def test_products_on_the_hub_case(dt, q):
    tdt, npdt = DT[dt]
    c, op = C.operator("hub")
    rng = np.random.default_rng(q)
    vals = np.stack([c["values"], rng.uniform(-1, 1, len(c["values"]))]).astype(npdt)
    u, w = rng.uniform(-1, 1, (2, c["m"], q)).astype(npdt), rng.uniform(-1, 1, (2, c["n"], q)).astype(npdt)
    if q == 1:
        u, w = u[..., 0], w[..., 0]
    jt = S.jt_vec(op, _dev(vals, tdt), _dev(u, tdt))
    jv = S.j_vec(op, _dev(vals, tdt), _dev(w, tdt))
    for b in range(2):
        want_t = N.ref_jt_vec(c["rows"], c["cols"], c["n"], vals[b], u[b], npdt)
        want_v = N.ref_j_vec(c["rows"], c["cols"], c["m"], vals[b], w[b], npdt)
        assert _bits(jt[b]) == _bits(want_t) and _bits(jv[b]) == _bits(want_v), (dt, q, b)
        # a member alone is the member of the batch
        assert _bits(S.jt_vec(op, _dev(vals[b], tdt), _dev(u[b], tdt))) == _bits(want_t)
        assert _bits(S.j_vec(op, _dev(vals[b], tdt), _dev(w[b], tdt))) == _bits(want_v)
    # the same bits and the same gradients as on a JacobianPattern
    pat = S.JacobianPattern(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
    grads = []
    for route in (op, pat, pat.operator):
        vv, uu = _dev(vals[0], tdt).requires_grad_(), _dev(u[0], tdt).requires_grad_()
        out = S.jt_vec(route, vv, uu)
        assert _bits(out) == _bits(jt[0])
        out.square().sum().backward()
        grads.append((vv.grad, uu.grad))
    for g in grads[1:]:
        assert _bits(g[0]) == _bits(grads[0][0]) and _bits(g[1]) == _bits(grads[0][1])


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_same_bits_for_every_check_every_column_and_batch(dt, precond):
    tdt, npdt = DT[dt]
    c, op = C.operator("blocks")
    rng = np.random.default_rng(11)
    vals = np.stack([c["values"] * s for s in (1.0, 0.7, 1.3)]).astype(npdt)
    r = rng.uniform(-1, 1, (3, c["m"], 3)).astype(npdt)
    r[1, :, 2] = 0.0
    v, rd = _dev(vals, tdt), _dev(r, tdt)
    kw = dict(damping=AB, precond=precond, tol=1e-6 if dt == "f64" else 1e-3, max_steps=40, return_info=True)
    x, info = S.lstsq_cg(op, v, rd, check_every=8, **kw)
    assert info["stop"][1, 2] == 5 and (info["stop"][0] == 1).all()
    for ce in (1, 3, None):
        x2, i2 = S.lstsq_cg(op, v, rd, check_every=ce, **kw)
        assert _bits(x2) == _bits(x) and _bits(i2["state"]) == _bits(info["state"]), ce
    for b in range(3):
        xb, ib = S.lstsq_cg(op, v[b], rd[b], **kw)
        assert _bits(xb) == _bits(x[b]) and _bits(ib["state"]) == _bits(info["state"][b]), b
        if precond is not None:
            assert _bits(ib["precond_status"]) == _bits(info["precond_status"][b])
        for j in range(3):
            xj, ij = S.lstsq_cg(op, v[b], rd[b, :, j].contiguous(), **kw)
            assert _bits(xj) == _bits(x[b, :, j]) and _bits(ij["state"]) == _bits(info["state"][b, j]), (b, j)
    want, st, _ = C.cgls_model(c, npdt, r=r[2], damping_ab=AB, precond=precond, tol=kw["tol"], max_steps=40, values=vals[2])
    _check(x[2], {"state": info["state"][2]}, want, st, None, "member 2")


def _iterate_by_pieces(run):
    """one iteration through the entries of the pieces: what bsp_cgls_iterate_* queues in one call"""
    from baspacho_amd import _call
    v, p, t = run._args("jv", run.values, run.p, run.t)
    _call(run._lib, "bsp_jac_product_jv_", run.batched, run.sfx, run.solver._h, run.product._h, v, p, run._q, t,
          *run._count)
    run._piece("delta", run._q, t, p, run._args("d", run.d)[0], run._work, run._state)
    run._piece("update", run._q, p, t, *run._args("xres", run.x, run.res), run._state)
    run._normal(True, run._state)
    run._direction(run._apply(False))


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi", "callable"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_fused_iteration_is_the_pieces(dt, precond):
    tdt, npdt = DT[dt]
    c, op, r, x0 = _operands("hub", npdt, q=3)
    vals = _dev(np.stack([c["values"], 0.8 * c["values"]]), tdt)
    rd, xd = _dev(np.stack([r, -r]), tdt), _dev(np.stack([x0, x0]), tdt)
    runs = []
    with _OnCurrentStream(op.solver, vals.device):
        csq = CGLS.column_norms(op.product, vals)
        d = CGLS.damping_vector(op.product, csq, AB[0], AB[1], vals)
        inv = (1.0 / (csq + d)).to(tdt)
        for fused in (True, False):
            pc = (lambda s: s * inv[..., None]) if precond == "callable" else \
                None if precond is None else CGLS.Preconditioner(op.product, precond, vals, csq, d)
            run = CGLS.CglsRun(op.product, vals, rd, None, d, xd.clone(), True, pc, 1e-10, 9)
            run.start()
            for _ in range(9):
                run.iterate() if fused else _iterate_by_pieces(run)
            runs.append(run)
    assert (runs[0].state[..., 0] == 9).all()
    for name in ("x", "res", "s", "p", "state"):
        assert _bits(getattr(runs[0], name)) == _bits(getattr(runs[1], name)), name


def test_frozen_column():
    # column 0 starts at the solution and stops converged at once; column 1 runs on beside it
    c, v = C.dense_case("scalar", 1.0)
    op = C.operator("scalar")[1]
    rng = np.random.default_rng(4)
    r = rng.uniform(-1, 1, (c["m"], 2))
    xd, _ = C.dense_solution(c, r=r, damping_ab=AB, values=v)
    x0 = np.stack([xd[:, 0], rng.uniform(-1, 1, c["n"])], axis=1)
    x, info = S.lstsq_cg(op, _dev(v, torch.float64), _dev(r, torch.float64), damping=AB, precond="jacobi", tol=1e-8,
                         max_steps=50, x0=_dev(x0, torch.float64), return_info=True)
    assert info["stop"].tolist() == [1, 1] and info["iterations"][0] == 0 and info["iterations"][1] > 3
    assert _bits(x[:, 0]) == _bits(x0[:, 0])
    want, st, status = C.cgls_model(c, np.float64, r=r, damping_ab=AB, precond="jacobi", tol=1e-8, max_steps=50, x0=x0,
                                    values=v)
    _check(x, info, want, st, status, "frozen")


@pytest.mark.parametrize("case", ["breakdown", "nan", "zero", "bad_block", "empty"])
def test_stops_and_status_on_the_device(case):
    c, op = C.operator("blocks")
    vals = c["values"].copy()
    rng = np.random.default_rng(2)
    r = rng.uniform(-1, 1, (c["m"], 2))
    col = 5
    tdt = torch.float64
    if case == "breakdown":
        # an all-zero column without damping: N is singular along e_col, the curvature of that direction is 0
        vals[c["cols"] == col] = 0.0
        cv = np.zeros((c["n"], 2))
        cv[col, 0] = 1.0
        cv[:, 1] = rng.uniform(-1, 1, c["n"])
        x, info = _solve(op, _dev(vals, tdt), c=_dev(cv, tdt), precond=None, max_steps=30)
        want, st, _ = C.cgls_model(c, np.float64, c=cv, precond=None, max_steps=30, values=vals)
        assert info["stop"][0] == 3 and info["iterations"][0] == 0 and st["pAp"][0] == 0.0
        _check(x, info, want, st, None, case)
    elif case == "nan":
        vals[7] = np.nan
        x, info = S.lstsq_cg(op, _dev(vals, tdt), _dev(r, tdt), precond="jacobi", return_info=True)
        assert info["stop"].tolist() == [4, 4] and info["iterations"].tolist() == [0, 0]
    elif case == "zero":
        r[:, 0] = 0.0
        x, info = S.lstsq_cg(op, _dev(vals, tdt), _dev(r, tdt), precond="block_jacobi", max_steps=40, return_info=True,
                             x0=_dev(rng.uniform(-1, 1, (c["n"], 2)), tdt))
        assert info["stop"].tolist() == [5, 1] and not x[:, 0].any() and info["relres"][0] == 0
    elif case == "bad_block":
        vals[c["cols"] == col] = 0.0
        x, info = S.lstsq_cg(op, _dev(vals, tdt), _dev(r, tdt), precond="block_jacobi", max_steps=12, return_info=True)
        want, st, status = C.cgls_model(c, np.float64, r=r, precond="block_jacobi", max_steps=12, values=vals)
        assert status.tolist() == [col, 1]
        _check(x, info, want, st, status, case)
        x, info = S.lstsq_cg(op, _dev(vals, tdt), _dev(r, tdt), precond="jacobi", max_steps=12, return_info=True)
        assert info["precond_status"].tolist() == [col, 1]
    else:
        ce, oe = C.operator("empty")
        x, info = S.lstsq_cg(oe, torch.zeros(0, dtype=tdt, device="cuda"), _dev(np.ones(ce["m"]), tdt), return_info=True)
        assert info["stop"] == 5 and not x.any() and info["precond_status"].tolist() == [0, 3]


@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,scale", C.DENSE_CASES)
def test_against_dense_float64_and_lstsq(name, scale, dt, precond):
    tdt, npdt = DT[dt]
    tol, bound = (1e-12, 1e-10) if dt == "f64" else (1e-6, 1e-4)
    c, vals = C.dense_case(name, scale)
    op = C.operator(name)[1]
    r = np.random.default_rng(5).uniform(-1, 1, (c["m"], 2))
    xd, Nm = C.dense_solution(c, r=r.astype(npdt), damping_ab=C.DENSE_DAMPING, values=vals.astype(npdt))
    assert np.linalg.cond(Nm) <= 100
    v, rd = _dev(vals, tdt), _dev(r, tdt)
    x, info = S.lstsq_cg(op, v, rd, damping=C.DENSE_DAMPING, precond=precond, tol=tol, max_steps=200, return_info=True)
    assert (info["stop"] == 1).all(), info["stop"]
    err = np.linalg.norm(x.cpu().numpy() - xd, axis=0) / np.linalg.norm(xd, axis=0)
    print("%s %s %s: iterations %s, error against dense %s" % (name, dt, precond, info["iterations"].tolist(), err))
    assert (err < bound).all(), err
    pat = N.pattern(name)[1]
    xl = S.lstsq(pat, v, rd, damping=C.DENSE_DAMPING)
    xp = S.lstsq_cg(pat, v, rd, damping=C.DENSE_DAMPING, precond=precond, tol=tol, max_steps=200)
    assert _bits(xp) == _bits(x)  # the pattern's operator, on the pattern's own solver
    diff = ((x - xl).norm(dim=0) / xl.norm(dim=0)).cpu().numpy()
    assert (diff < bound).all(), diff


def test_gradients():
    c = C.case("scalar_small")
    assert c["n"] <= 12
    op = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=[3, 1, 2, 3, 3])
    rng = np.random.default_rng(8)
    v = _dev(c["values"], torch.float64).requires_grad_()
    r = _dev(rng.uniform(-1, 1, (c["m"], 2)), torch.float64).requires_grad_()
    alpha = torch.tensor(0.3, dtype=torch.float64, device="cuda", requires_grad=True)
    beta = torch.tensor(0.2, dtype=torch.float64, device="cuda", requires_grad=True)
    for precond in (None, "block_jacobi"):
        f = lambda v, r, alpha, beta: S.lstsq_cg(op, v, r, damping=(alpha, beta), precond=precond, tol=1e-13, max_steps=200)
        assert torch.autograd.gradcheck(f, (v, r, alpha, beta), eps=1e-6, atol=1e-7, rtol=1e-6)
    # a batch, a single right-hand side, no damping
    vb = torch.stack([v.detach(), 1.1 * v.detach()]).requires_grad_()
    rb = torch.stack([r.detach()[:, 0], r.detach()[:, 1]]).requires_grad_()
    f = lambda v, r: S.lstsq_cg(op, v, r, precond="jacobi", tol=1e-13, max_steps=200)
    assert torch.autograd.gradcheck(f, (vb, rb), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_framed_and_offset_operands(dt):
    tdt, npdt = DT[dt]
    c, op, r, x0 = _operands("hub", npdt, q=3)
    nb = 2
    vals = np.stack([c["values"], 0.9 * c["values"]]).astype(npdt)
    rr, xx = np.stack([r, 0.5 * r]), np.stack([x0, -x0])
    plain = S.lstsq_cg(op, _dev(vals, tdt), _dev(rr, tdt), damping=AB, precond="block_jacobi", max_steps=10,
                       x0=_dev(xx, tdt), return_info=True)
    # every operand inside its own guards, at an odd element offset: element-aligned, never 16-byte-aligned
    fr = framed(npdt, [vals, rr, xx])
    fv, frr, fx = (fr.view(k).reshape(a.shape) for k, a in enumerate((vals, rr, xx)))
    assert all(t.data_ptr() % 16 != 0 for t in (fv, frr, fx))
    x, info = S.lstsq_cg(op, fv, frr, damping=AB, precond="block_jacobi", max_steps=10, x0=fx, return_info=True)
    fr.assert_intact(read_only=(0, 1, 2), what="lstsq_cg")
    assert _bits(x) == _bits(plain[0]) and _bits(info["state"]) == _bits(plain[1]["state"])
    # the driver's own vectors framed as well: x is written in place, everything else stays inside its payload
    with _OnCurrentStream(op.solver, fv.device):
        csq = CGLS.column_norms(op.product, fv)
        d = CGLS.damping_vector(op.product, csq, AB[0], AB[1], fv)
        pc = CGLS.Preconditioner(op.product, "block_jacobi", fv, csq, d)
        f2 = framed(npdt, [xx, d.cpu().numpy(), pc.values.cpu().numpy()])
        gx, gd, gm = (f2.view(k).reshape(s) for k, s in enumerate((xx.shape, d.shape, pc.values.shape)))
        pc.values = gm
        run = CGLS.CglsRun(op.product, fv, frr, None, gd, gx, True, pc, 1e-10, 10)
        shapes = {k: getattr(run, k).shape for k in ("res", "t", "s", "p", "z")}
        f3 = framed(npdt, [np.zeros(tuple(s), dtype=npdt) for s in shapes.values()])
        for k, name in enumerate(shapes):
            setattr(run, name, f3.view(k).reshape(shapes[name]))
        run.run(8)
    torch.cuda.synchronize()
    fr.assert_intact(read_only=(0, 1, 2), what="CglsRun")
    f2.assert_intact(read_only=(1, 2), what="CglsRun")
    f3.assert_intact(what="CglsRun")
    assert _bits(gx) == _bits(plain[0]) and _bits(run.state) == _bits(plain[1]["state"])


def test_a_veteran_operator_gives_the_bits_of_a_fresh_one():
    c = C.hub()
    make = lambda: S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
    rng = np.random.default_rng(12)
    r = rng.uniform(-1, 1, (c["m"], 2))

    def probe(op):
        out = []
        for dt, precond in (("f64", "block_jacobi"), ("f32", "jacobi"), ("f64", None)):
            tdt = DT[dt][0]
            x, info = S.lstsq_cg(op, _dev(c["values"], tdt), _dev(r, tdt), damping=AB, precond=precond, max_steps=9,
                                 return_info=True)
            out.append(_bits(x) + _bits(info["state"]) + _bits(info.get("precond_status", torch.zeros(0))))
            out.append(_bits(S.jt_vec(op, _dev(c["values"], tdt), _dev(r, tdt))))
        return out

    veteran = make()
    for dt, nb, q in (("f32", 3, 1), ("f64", 1, 4), ("f32", 2, 2)):
        tdt = DT[dt][0]
        vals = _dev(np.stack([c["values"] * (1 + 0.1 * b) for b in range(nb)]), tdt)
        rb = _dev(rng.uniform(-1, 1, (nb, c["m"], q)), tdt)
        S.j_vec(veteran, vals, S.jt_vec(veteran, vals, rb))
        for precond in ("jacobi", None, "block_jacobi"):
            S.lstsq_cg(veteran, vals, rb, damping=None if precond is None else AB, precond=precond, max_steps=5,
                       check_every=None)
    assert probe(veteran) == probe(make())


def test_refusals():
    c, op = C.operator("scalar")
    tdt = torch.float64
    v, r = _dev(c["values"], tdt), _dev(np.ones(c["m"]), tdt)
    with pytest.raises(TypeError, match="pattern must be a JacobianPattern or a JacobianOperator"):
        S.lstsq_cg(None, v, r)
    with pytest.raises(ValueError, match=r"values must be \[%d\] or \[B, %d\]" % (op.nnz, op.nnz)):
        S.lstsq_cg(op, v[:-1], r)
    with pytest.raises(TypeError, match="values must be float64 or float32"):
        S.lstsq_cg(op, v.half(), r)
    with pytest.raises(ValueError, match="values must live in device memory"):
        S.lstsq_cg(op, v.cpu(), r)
    with pytest.raises(TypeError, match="r has dtype torch.float32, jvalues have torch.float64"):
        S.lstsq_cg(op, v, r.float())
    with pytest.raises(ValueError, match=r"r must be \[rows\] or \[rows, q\] with %d rows" % op.m):
        S.lstsq_cg(op, v, r[:-1])
    with pytest.raises(ValueError, match=r"r must be \[B, rows\] or \[B, rows, q\]"):
        S.lstsq_cg(op, torch.stack([v, v]), r)
    with pytest.raises(ValueError, match="tol must be a number >= 0"):
        S.lstsq_cg(op, v, r, tol=-1e-3)
    with pytest.raises(ValueError, match="max_steps must be an integer >= 0"):
        S.lstsq_cg(op, v, r, max_steps=-1)
    with pytest.raises(ValueError, match="check_every must be None or an integer >= 1"):
        S.lstsq_cg(op, v, r, check_every=0)
    with pytest.raises(ValueError, match="precond must be None, 'jacobi', 'block_jacobi' or a callable"):
        S.lstsq_cg(op, v, r, precond="fsai")
    with pytest.raises(TypeError, match=r"damping must be a pair \(alpha, beta\)"):
        S.lstsq_cg(op, v, r, damping=0.1)
    with pytest.raises(ValueError, match="damping alpha must be a float or a 0-dim tensor"):
        S.lstsq_cg(op, v, r, damping=(torch.ones(2), 0.1))
    with pytest.raises(ValueError, match=r"x0 must be a torch.float64 tensor of shape \(%d,\)" % op.n):
        S.lstsq_cg(op, v, r, x0=torch.zeros(op.n + 1, dtype=tdt, device="cuda"))
    wide = S.JacobianOperator([0, 1], [0, 40], 2, 41, param_sizes=[8, 33])
    with pytest.raises(ValueError, match="param 1 has 33 scalars; 'block_jacobi' takes params of at most 32"):
        S.lstsq_cg(wide, _dev(np.ones(2), tdt), _dev(np.ones(2), tdt))
    assert S.lstsq_cg(wide, _dev(np.ones(2), tdt), _dev(np.ones(2), tdt), precond="jacobi").shape == (41,)
    with pytest.raises(ValueError, match="r and c cannot both be absent"):
        _solve(op, v)
    with pytest.raises(ValueError, match="must return a tensor of shape"):
        S.lstsq_cg(op, v, r, precond=lambda s: s[:-1])
    # a callable preconditioner is the built-in one when it computes the same thing
    with _OnCurrentStream(op.solver, v.device):
        inv = 1.0 / CGLS.column_norms(op.product, v)
    x1, i1 = S.lstsq_cg(op, v, r, precond="jacobi", return_info=True)
    x2, i2 = S.lstsq_cg(op, v, r, precond=lambda s: s * inv, return_info=True)
    assert _bits(x1) == _bits(x2) and _bits(i1["state"]) == _bits(i2["state"])
    # the C entries refuse what the pieces need and do not get
    lib, P, I64 = op.solver._lib, __import__("ctypes").c_void_p, __import__("ctypes").c_int64
    assert lib.bsp_cgls_init_f64(op.solver._h, op.product._h, I64(1), None, None, __import__("ctypes").c_double(0.0),
                                 I64(1), None, None) != 0
    assert "cglsInit: the workspace pointer is NULL" in lib.bsp_last_error().decode()
    other = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"])
    assert lib.bsp_jac_product_jv_f64(other.solver._h, op.product._h, P(v.data_ptr()), P(v.data_ptr()), I64(1),
                                      P(v.data_ptr())) != 0
    assert "the map was built on another solver" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_product_jv_f64(op.solver._h, op.product._h, P(v.data_ptr()), None, I64(1), P(v.data_ptr())) != 0
    assert "cglsJv: the vector pointer of batch member 0 is NULL" in lib.bsp_last_error().decode()
