"""GPU: the block diagonal of the reduced matrix S as preconditioner ("schur_jacobi") on the
MI355X.  schurJacobiBuild must be bitwise the numpy restatement (schur_jacobi_ref.py) -- the inverses, the chunk
partials and the status record -- in f64 and f32, with and without damping, on schur_ref's cases and the case of the
chunk and pseudo-pair edges, for a batch of 2, with framed, poisoned and offset buffers; schurJacobiApply is bitwise
the kind-2 apply on the same inverses and never builds the kept item plan; lstsq_cg(eliminate=...,
precond="schur_jacobi") is bitwise the model's solve (x, the records, both status records), reaches the dense solution
within kappa(N) tol, passes gradcheck and gives the same bits from a veteran map as from a fresh one."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from baspacho_amd import cgls as CGLS
from baspacho_amd import sparse as S
from baspacho_amd.autograd import _OnCurrentStream
from buffer_edges import SENTINEL_BITS, Frame, framed
import cg_ref as R
import cgls_ref as C
import schur_jacobi_ref as J
import schur_ref as SR

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
AB = J.DAMPING


def _dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _damping(jop, v, damped):
    return CGLS.damping_vector(jop.product, CGLS.column_norms(jop.product, v), AB[0], AB[1], v) if damped else None


@functools.lru_cache(maxsize=None)
def _vectors(name, npdt, q):
    c, _ = J.case(name)
    rng = np.random.default_rng(q + c["m"])
    return rng.uniform(-1, 1, (c["m"], q)).astype(npdt), rng.uniform(-1, 1, (c["n"], q)).astype(npdt)


# ---- the build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", J.CASES)
def test_build_bitwise_against_the_restatement(name, dt):
    """minv, the status and every chunk partial; the partials lie in a frame full of the sentinel: nothing outside them
    is written, and the block kernel, which reads every element of them, meets no sentinel"""
    tdt, npdt = DT[dt]
    c, elim, jop, sch = J.operator(name)
    v = _dev(c["values"], tdt)
    for damped in (False, True):
        mdl, pc = J.model(name, npdt, damped)
        with _OnCurrentStream(jop.solver, v.device):
            d = _damping(jop, v, damped)
            binv, estatus = sch.map.build(v, d)
            assert _bits(binv[:len(mdl.binv)]) == _bits(mdl.binv) and estatus.tolist() == mdl.status.tolist()
            fr = Frame([max(len(pc.partials), 1)], np.float64)
            minv, status = sch.map.schurJacobiBuild(v, binv, d, partials=fr.view(0))
        torch.cuda.synchronize()
        fr.assert_intact(what="partials")
        part = fr.host(0)[:len(pc.partials)]
        assert not (part.view(np.uint64) == np.uint64(SENTINEL_BITS[np.float64])).any(), "a partial was never written"
        assert _bits(part) == _bits(pc.partials), (name, dt, damped, "partials")
        assert minv.dtype == tdt and _bits(minv[:len(pc.minv)]) == _bits(pc.minv), (name, dt, damped, "minv")
        np.testing.assert_array_equal(status.cpu().numpy(), pc.status, err_msg=str((name, dt, damped)))
    info = sch.map.schurJacobiInfo()
    assert info["inverse_elems"] == len(pc.minv) and info["partial_elems"] == len(pc.partials)


def test_the_bad_blocks_are_reported():
    """the edges case without damping: the kept param without rows is a zero block, its inverse zero and its first
    scalar the status; the eliminated param with zero values has a zero inverse, so that its pair adds G alone"""
    c, elim, jop, sch = J.operator("edges")
    mdl, pc = J.model("edges", np.float64, False)
    v = _dev(c["values"], torch.float64)
    with _OnCurrentStream(jop.solver, v.device):
        binv, estatus = sch.map.build(v)
        minv, status = sch.map.schurJacobiBuild(v, binv)
    t = J.plan("edges")
    assert estatus.tolist() == [int(mdl.t["elim_scalar"][-1]), 1]
    assert status.tolist() == [int(t["kept_first"][-1]), 1] == pc.status.tolist()
    assert not minv[int(t["block_off"][-2]):].any() and minv[:int(t["block_off"][-2])].abs().min() > 0


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["ba", "edges"])
def test_a_batch_of_two_is_its_members(name, dt):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = J.operator(name)
    vals = np.stack([c["values"], 0.9 * c["values"]]).astype(npdt)
    v = _dev(vals, tdt)
    with _OnCurrentStream(jop.solver, v.device):
        d = _damping(jop, v, True)
        binv, _ = sch.map.build(v, d)
        minv, status = sch.map.schurJacobiBuild(v, binv, d)
        for b in range(2):
            m1, s1 = sch.map.schurJacobiBuild(v[b], binv[b], d[b])
            assert _bits(m1) == _bits(minv[b]) and _bits(s1) == _bits(status[b]), (name, dt, b)
    mdl = SR.Model(c, elim, npdt, values=vals[1], damping_ab=AB, t=J.model(name, npdt, True)[0].t)
    pc = J.Precond(mdl, J.plan(name))
    assert _bits(minv[1, :len(pc.minv)]) == _bits(pc.minv) and status[1].tolist() == pc.status.tolist()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_framed_and_offset_buffers(dt):
    """values, binv and d inside guards at odd element offsets (never 16-byte aligned), minv and the partials framed:
    the operands are not written, nothing outside the outputs is, and the bits are those of plain buffers"""
    tdt, npdt = DT[dt]
    c, elim, jop, sch = J.operator("edges")
    vals = np.stack([c["values"], 0.9 * c["values"]]).astype(npdt)
    v = _dev(vals, tdt)
    info = sch.map.schurJacobiInfo()
    with _OnCurrentStream(jop.solver, v.device):
        d = _damping(jop, v, True)
        binv, _ = sch.map.build(v, d)
        want, wstatus = sch.map.schurJacobiBuild(v, binv, d)
        fin = framed(npdt, [vals, binv.cpu().numpy(), d.cpu().numpy()])
        fv, fb, fd = (fin.view(k).reshape(s) for k, s in enumerate((vals.shape, binv.shape, d.shape)))
        assert all(t.data_ptr() % 16 != 0 for t in (fv, fb, fd))
        fout = Frame([2 * info["inverse_elems"]], npdt)
        fpart = Frame([2 * info["partial_elems"]], np.float64)
        out = fout.view(0).reshape(2, info["inverse_elems"])
        minv, status = sch.map.schurJacobiBuild(fv, fb, fd, partials=fpart.view(0).reshape(2, -1), out=out)
    torch.cuda.synchronize()
    fin.assert_intact(read_only=(0, 1, 2), what="schurJacobiBuild operands")
    fout.assert_intact(what="minv")
    fpart.assert_intact(what="partials")
    assert minv.data_ptr() == out.data_ptr() and _bits(minv) == _bits(want) and _bits(status) == _bits(wstatus)


# ---- the apply ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("batch", [None, 2])
def test_apply_is_the_kind_2_apply_and_needs_no_kept_item_plan(dt, batch):
    tdt, npdt = DT[dt]
    c, elim = J.case("w8")
    jop = S.JacobianOperator(c["rows"], c["cols"], c["m"], c["n"], param_sizes=c["param_sizes"])
    sch = S.JacobianSchur(jop, np.asarray(elim, dtype=np.int64))
    sm, lib, q = sch.map, sch.map._lib, 3
    lead = () if batch is None else (batch,)
    vals = c["values"] if batch is None else np.stack([c["values"] * (1 - 0.1 * b) for b in range(batch)])
    v = _dev(vals, tdt)
    rng = np.random.default_rng(3)
    r = _dev(rng.uniform(-1, 1, lead + (sch.nK, q)), tdt)
    before = sm.info()
    need = ctypes.c_int64(0)
    assert lib.bsp_cg_work_bytes(jop.solver._h, ctypes.c_int64(sch.nK), ctypes.c_int64(q), ctypes.byref(need)) == 0
    nb = 1 if batch is None else batch
    outs = []
    with _OnCurrentStream(jop.solver, v.device):
        d = _damping(jop, v, True)
        binv, _ = sm.build(v, d)
        minv, _ = sm.schurJacobiBuild(v, binv, d)
        for kind2 in (False, True):
            work = torch.zeros(need.value * nb + 16, dtype=torch.uint8, device="cuda")
            wptr = ctypes.c_void_p((work.data_ptr() + 15) // 16 * 16)
            state = torch.zeros(lead + (q, 12), dtype=torch.int64, device="cuda")  # running records, iteration 0
            z = torch.full_like(r, float("nan"))
            if not kind2:
                sm.schurJacobiApply(minv, r, z, wptr, state)
                assert sm.schurJacobiInfo()["kept_item_plan_built"] is False and sm.info() == before
            else:
                mem = lambda t: sm._members(t, batch is not None)
                fn = getattr(lib, "bsp_jac_schur_precond_apply_" + ("batched_" if batch else "") + dt)
                assert fn(jop.solver._h, sm._h, ctypes.c_int32(2), ctypes.c_int64(q), mem(minv), mem(r), mem(z), wptr,
                          ctypes.c_void_p(state.data_ptr()), *((ctypes.c_int32(batch),) if batch else ())) == 0
                assert sm.schurJacobiInfo()["kept_item_plan_built"] is True
            torch.cuda.synchronize()
            outs.append((_bits(z), _bits(state)))
            assert not torch.isnan(z).any() and (state[..., 2].view(torch.float64) > 0).all()  # r.z of a positive block
    assert outs[0] == outs[1]
    # the restatement's apply, on member 0
    mdl = SR.Model(c, elim, npdt, values=np.asarray(vals).reshape(nb, -1)[0], damping_ab=AB)
    pc = J.Precond(mdl, J.plan("w8"))
    r0 = r.cpu().numpy().reshape((nb, sch.nK, q))[0]
    z0 = np.frombuffer(outs[0][0], dtype=npdt).reshape((nb, sch.nK, q))[0]
    assert _bits(z0) == _bits(pc.apply(r0))


# ---- the reduced solve ----------------------------------------------------------------------------------------
def _solve(sch, v, r=None, c=None, ab=None, tol=1e-10, max_steps=10, x0=None):
    cache = {}
    with _OnCurrentStream(sch.jop.solver, v.device):
        x, run = S._schur_run(sch, v, r, c, ab, "schur_jacobi", tol, max_steps, 8, x0, cache)
    return x, {"state": run.state, "eliminate_status": cache["eliminate_status"],
               "precond_status": cache["schur_jacobi"].status}


def _check(got_x, info, want_x, st, estatus, pstatus, what):
    assert _bits(got_x) == _bits(want_x), (what, "x", np.abs(got_x.cpu().numpy() - want_x).max())
    state = info["state"].cpu().numpy().reshape(-1, 12)
    for j in range(state.shape[0]):
        np.testing.assert_array_equal(state[j], R.record_words(st, j), err_msg="%s column %d" % (what, j))
    np.testing.assert_array_equal(info["eliminate_status"].cpu().numpy(), estatus, err_msg=str(what))
    np.testing.assert_array_equal(info["precond_status"].cpu().numpy(), pstatus, err_msg=str(what))


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", J.CASES)
def test_solve_bitwise_against_the_restatement(name, dt, q):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = J.operator(name)
    v = _dev(c["values"], tdt)
    r, cv = _vectors(name, npdt, q)
    for damped in ((True,) if name in ("hub", "edges") else (False, True)):  # (those are singular without damping)
        mdl, pc = J.model(name, npdt, damped)
        for which, kw in (("r", dict(r=r)), ("c", dict(c=cv)), ("rc", dict(r=r, c=cv)), ("x0", dict(r=r, x0=cv))):
            want, st = mdl.solve(precond=pc.apply, max_steps=10, **kw)
            got, info = _solve(sch, v, ab=AB if damped else None, **{k: _dev(a, tdt) for k, a in kw.items()})
            _check(got, info, want, st, mdl.status, pc.status, (name, dt, q, damped, which))
    # the public entry: the same bits and records (the last run: r and x0, damped); [rows] operands for q = 1
    rd, x0 = (_dev(a[:, 0] if q == 1 else a, tdt) for a in (r, cv))
    x, info = S.lstsq_cg(jop, v, rd, damping=AB, precond="schur_jacobi", max_steps=10, x0=x0, return_info=True,
                         eliminate=sch)
    assert x.shape == x0.shape
    _check(x.reshape(want.shape), info, want, st, mdl.status, pc.status, (name, dt, q, "lstsq_cg"))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_a_batch_of_two_solves_is_its_members(dt):
    tdt, npdt = DT[dt]
    c, elim, jop, sch = J.operator("ba")
    vals = np.stack([c["values"], 0.8 * c["values"]]).astype(npdt)
    r, _ = _vectors("ba", npdt, 3)
    rr = np.stack([r, -0.5 * r]).astype(npdt)
    kw = dict(damping=AB, precond="schur_jacobi", max_steps=10, return_info=True, eliminate=sch)
    x, info = S.lstsq_cg(jop, _dev(vals, tdt), _dev(rr, tdt), **kw)
    for b in range(2):
        xb, ib = S.lstsq_cg(jop, _dev(vals[b], tdt), _dev(rr[b], tdt), **kw)
        assert _bits(xb) == _bits(x[b]) and _bits(ib["state"]) == _bits(info["state"][b])
        assert _bits(ib["precond_status"]) == _bits(info["precond_status"][b])
        mdl = SR.Model(c, elim, npdt, values=vals[b], damping_ab=AB, t=J.model("ba", npdt, True)[0].t)
        pc = J.Precond(mdl, J.plan("ba"))
        want, st = mdl.solve(r=rr[b], precond=pc.apply, max_steps=10)
        _check(x[b], {k: info[k][b] for k in ("state", "eliminate_status", "precond_status")}, want, st, mdl.status,
               pc.status, ("member", b))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", SR.DENSE_CASES)
def test_against_the_dense_solution(name, dt):
    """the CPU test's bound: kappa(N) tol on the relative error of the full x, kappa(N) <= 100 from the dense matrix"""
    tdt, npdt = DT[dt]
    tol = 1e-12 if dt == "f64" else 1e-6
    c, elim, jop, sch = J.operator(name)
    r = np.random.default_rng(5).uniform(-1, 1, (c["m"], 2)).astype(npdt)
    xd, Nm = C.dense_solution(c, r=r, damping_ab=AB, values=c["values"].astype(npdt))
    kappa = np.linalg.cond(Nm)
    assert kappa <= 100
    x, info = S.lstsq_cg(jop, _dev(c["values"], tdt), _dev(r, tdt), damping=AB, precond="schur_jacobi", tol=tol,
                         max_steps=200, return_info=True, eliminate=sch)
    assert (info["stop"] == 1).all() and info["precond_status"].tolist() == [-1, 0]
    err = np.linalg.norm(x.cpu().numpy().astype(np.float64) - xd, axis=0) / np.linalg.norm(xd, axis=0)
    print("%s %s: kappa %.1f, iterations %s, error %s, bound %.1e" % (name, dt, kappa, info["iterations"].tolist(), err,
                                                                     kappa * tol))
    assert (err <= kappa * tol).all(), (err, kappa * tol)


def test_gradients():
    c, elim, jop, sch = SR.operator("tiny")
    rng = np.random.default_rng(8)
    v = _dev(c["values"], torch.float64).requires_grad_()
    r = _dev(rng.uniform(-1, 1, (c["m"], 2)), torch.float64).requires_grad_()
    alpha = torch.tensor(0.3, dtype=torch.float64, device="cuda", requires_grad=True)
    beta = torch.tensor(0.2, dtype=torch.float64, device="cuda", requires_grad=True)
    f = lambda v, r, alpha, beta: S.lstsq_cg(jop, v, r, damping=(alpha, beta), precond="schur_jacobi", tol=1e-13,
                                             max_steps=200, eliminate=sch)
    assert torch.autograd.gradcheck(f, (v, r, alpha, beta), eps=1e-6, atol=1e-7, rtol=1e-6)
    vb = torch.stack([v.detach(), 1.1 * v.detach()]).requires_grad_()
    rb = torch.stack([r.detach()[:, 0], r.detach()[:, 1]]).requires_grad_()
    f = lambda v, r: S.lstsq_cg(jop, v, r, precond="schur_jacobi", tol=1e-13, max_steps=200, eliminate=sch)
    assert torch.autograd.gradcheck(f, (vb, rb), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_a_veteran_map_gives_the_bits_of_a_fresh_one():
    c, elim = J.case("edges")
    jop = J.operator("edges")[2]
    make = lambda: S.JacobianSchur(jop, np.asarray(elim))
    rng = np.random.default_rng(12)
    r = rng.uniform(-1, 1, (c["m"], 2))

    def probe(sch):
        out = []
        for dt, ab in (("f64", AB), ("f32", AB), ("f64", (0.0, 0.5))):
            tdt = DT[dt][0]
            x, info = S.lstsq_cg(jop, _dev(c["values"], tdt), _dev(r, tdt), damping=ab, precond="schur_jacobi", max_steps=6,
                                 return_info=True, eliminate=sch)
            out.append(_bits(x) + _bits(info["state"]) + _bits(info["eliminate_status"]) + _bits(info["precond_status"]))
        return out

    veteran = make()
    vals = _dev(np.stack([c["values"] * (1 + 0.1 * b) for b in range(2)]), torch.float32)
    rb = _dev(rng.uniform(-1, 1, (2, c["m"], 2)), torch.float32)
    for precond in ("block_jacobi", "jacobi", None):
        S.lstsq_cg(jop, vals, rb, damping=AB, precond=precond, max_steps=5, check_every=None, eliminate=veteran)
    first = probe(veteran)
    S.lstsq_cg(jop, vals, rb, damping=AB, precond="block_jacobi", max_steps=5, eliminate=veteran)  # ... and after
    assert first == probe(veteran) == probe(make())


def test_refusals_of_lstsq_cg():
    c, elim, jop, sch = J.operator("w1")
    tdt = torch.float64
    v, r = _dev(c["values"], tdt), _dev(np.ones(c["m"]), tdt)
    with pytest.raises(ValueError, match="'schur_jacobi' is the block diagonal of the reduced system and needs eliminate"):
        S.lstsq_cg(jop, v, r, precond="schur_jacobi")
    with pytest.raises(ValueError, match="precond must be None, 'jacobi', 'block_jacobi' or a callable"):
        S.lstsq_cg(jop, v, r, precond="schur", eliminate=sch)
    with pytest.raises(ValueError, match="precond must be None, 'jacobi', 'block_jacobi' or a callable"):
        S.lstsq_cg(jop, v, r, precond="fsai")
    wide = S.JacobianOperator([0, 1], [0, 40], 2, 42, param_sizes=[8, 33, 1])
    ones = _dev(np.ones(2), tdt)
    with pytest.raises(ValueError, match="param 1 has 33 scalars; 'schur_jacobi' takes params of at most 32"):
        S.lstsq_cg(wide, ones, ones, precond="schur_jacobi", eliminate=[0])
    with _OnCurrentStream(jop.solver, v.device):
        binv, _ = sch.map.build(v)
        with pytest.raises(ValueError, match="binv must be what build\\(\\) returned"):
            sch.map.schurJacobiBuild(v, binv[:-1])
        with pytest.raises(ValueError, match="partials must be a float64 tensor of shape"):
            sch.map.schurJacobiBuild(v, binv, partials=torch.zeros(1, dtype=torch.float32, device="cuda"))
        minv, _ = sch.map.schurJacobiBuild(v, binv)
        z = torch.zeros(sch.nK, 1, dtype=tdt, device="cuda")
        with pytest.raises(ValueError, match="state must be the int64 records"):
            sch.map.schurJacobiApply(minv, z, z.clone(), 16, torch.zeros(2, 12, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="r must be a torch.float64 tensor"):
            sch.map.schurJacobiApply(minv, z[:-1], z.clone(), 16, torch.zeros(1, 12, dtype=torch.int64, device="cuda"))
    # the other choices give what they gave: the new string changes nothing beside itself
    x1 = S.lstsq_cg(jop, v, r, precond="block_jacobi", eliminate=sch)
    S.lstsq_cg(jop, v, r, precond="schur_jacobi", eliminate=sch)
    assert _bits(S.lstsq_cg(jop, v, r, precond="block_jacobi", eliminate=sch)) == _bits(x1)
