"""GPU: the "fsai" preconditioner of the device-resident conjugate gradient (kind 3) on
the MI355X.  The build (G and its status), the two products of the apply (t, z) and their r.z in the record must
be bitwise the numpy restatement (fsai_ref.py), in f64 and f32, single and in batches of 1 and 3, at the chunk
edges of the reduction, on rows of every width with truncation, on column lists at and over the long-run
threshold, with duplicates and "full" input; sparse.solve_cg(precond="fsai") bitwise the restated iteration;
stopped columns frozen; a bad row zeroed and reported; gradients against S.solve; no dependence on what the
product built before; the entries on framed, poisoned, element-aligned buffers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from baspacho_amd import cg as CG
from baspacho_amd import sparse as S
import buffer_edges as BE
import cg_ref as R
import fsai_ref as F
from test_cg_cpu import _plan_case

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64, 1e-8), "f32": (torch.float32, np.float32, 1e-4)}
NS = [1, 255, 1023, 1024, 1025, 2049]


def _dev(a, tdt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda()


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes()


def _values3(rows, cols, seed, diag):
    """three sets of values: a dominant diagonal (where the pattern has one) and small off-diagonal entries"""
    rng = np.random.default_rng(seed)
    on = rows == cols
    return np.stack([np.where(on, diag + rng.uniform(0, 1, len(rows)), rng.uniform(-1, 1, len(rows))) for _ in range(3)])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(n, rows, cols, triangle, values [3, nnz], the pattern, the restated plan)"""
    if isinstance(name, int):  # a chain with steps of 1 and 7 and every 5th diagonal entry given twice
        n = name
        d = np.arange(n, dtype=np.int64)
        dup = d[::5]
        rows, cols = np.concatenate([d, d[1:], d[7:], dup]), np.concatenate([d, d[:-1], d[:-7], dup])
        tri, diag = "lower", 4.0
    elif name in ("dups", "full"):
        n, rows, cols, _, tri = _plan_case(name)
        diag = 40.0  # (the diagonal is not everywhere in the pattern: those rows have a bad pivot)
    elif name == "banded33":
        n = 80
        rows, cols, _ = F.banded(n)
        tri, diag = "lower", 67.0
    else:
        n, rows, cols, _ = F.hub(int(name[3:]))
        tri, diag = "lower", 70.0
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    values = _values3(rows, cols, n + len(rows), diag)
    return n, rows, cols, tri, values, S.SymmetricPattern(rows, cols, n, triangle=tri), F.plan(n, rows, cols, tri)


def _start(pat, vd, bd, pc):
    """the first z of a solve from x = 0: init, the fsai apply and the direction; the CgRun"""
    run = CG.CgRun(pat.solver, bd, torch.zeros_like(bd), bd.clone(), lambda p, ap: ap, pc, 1e-10, 5)
    run.start()
    return run


def _check_pieces(name, q, dt):
    tdt, npdt, _ = DT[dt]
    n, rows, cols, tri, values, pat, pl = _case(name)
    rng = np.random.default_rng(q)
    b = rng.uniform(-1, 1, (3, n, q))
    if q > 1:
        b[1, :, 1] = 0.0  # a column that never starts: its t and z stay as allocated
    vd, bd = _dev(values, tdt), _dev(b, tdt)
    pcs = {"batch3": CG.Preconditioner(pat.product, "fsai", vd),
           "batch1": CG.Preconditioner(pat.product, "fsai", vd[:1]),
           "single": CG.Preconditioner(pat.product, "fsai", vd[0])}
    runs = {"batch3": _start(pat, vd, bd, pcs["batch3"]), "batch1": _start(pat, vd[:1], bd[:1], pcs["batch1"]),
            "single": _start(pat, vd[0], bd[0], pcs["single"])}
    torch.cuda.synchronize()
    elems = int(pl["row_start"][-1])
    bad_rows = 0
    for m in range(3):
        G, status = F.build(pl, values[m], npdt)
        bad_rows += int(status[1])
        r = b[m].astype(npdt)
        t, z = F.apply(pl, G, r)
        live = np.abs(r).sum(0) > 0
        t, z = np.where(live, t, 0).astype(npdt), np.where(live, z, 0).astype(npdt)
        rz = R.dot(r, z)
        for key in ("batch3", "batch1", "single")[:3 if m == 0 else 1]:
            pc, run = pcs[key], runs[key]
            pick = (lambda a: a[m]) if key != "single" else (lambda a: a)
            what = (name, q, dt, key, m)
            assert pick(pc.values).shape[-1] == max(elems, 1)
            assert _bits(pick(pc.values)[:elems]) == _bits(G), (what, "G")
            np.testing.assert_array_equal(pick(pc.status).cpu().numpy(), status, err_msg=str(what))
            assert _bits(pick(run.t)) == _bits(t), (what, "t")
            assert _bits(pick(run.z)) == _bits(z), (what, "z")
            state = pick(run.state).cpu().numpy()
            for j in range(q):
                rec = CG.read_state(torch.from_numpy(state[j]))
                if not live[j]:
                    assert rec["stop"] == R.ZERO_RHS
                    continue
                assert np.float64(rec["rz"]).tobytes() == np.float64(rz[j]).tobytes(), (what, "rz", j)
                assert rec["beta"] == 0.0 and rec["iterations"] == 0
                assert rec["stop"] == (R.RUNNING if rz[j] > 0 else R.BREAKDOWN)
    return bad_rows


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_build_and_apply_bitwise_at_the_chunk_edges(n, q, dt):
    assert _check_pieces(n, q, dt) == 0


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", ["banded33", "hub63", "hub64", "hub65", "dups", "full"])
def test_build_and_apply_bitwise_on_every_shape(name, dt):
    bad = _check_pieces(name, 3, dt)
    pl = _case(name)[6]
    assert (bad > 0) == (name in ("dups", "full"))
    if name == "banded33":
        assert sorted(set(np.diff(pl["row_start"]).tolist())) == list(range(1, 33))
    if name.startswith("hub"):
        assert len(pl["long_cols"]) == (1 if int(name[3:]) + 1 > 64 else 0)


# ---- the whole solve ----------------------------------------------------------------------------------------
def _check_solve(n, rows, cols, values, b, sizes, dt, max_steps):
    tdt, npdt, tol = DT[dt]
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes)
    x, info = S.solve_cg(pat, _dev(values, tdt), _dev(b, tdt), precond="fsai", tol=tol, max_steps=max_steps,
                         return_info=True)
    want, st, status = F.entries_model(n, rows, cols, values, b, npdt, tol=tol, max_steps=max_steps)
    assert _bits(x) == _bits(want)
    state = info["state"].cpu().numpy().reshape(-1, 12)
    for j in range(state.shape[0]):
        np.testing.assert_array_equal(state[j], R.record_words(st, j), err_msg="column %d" % j)
    np.testing.assert_array_equal(info["stop"].cpu().numpy().reshape(-1), st["stop"])
    np.testing.assert_array_equal(info["iterations"].cpu().numpy().reshape(-1), st["iterations"])
    np.testing.assert_array_equal(info["precond_status"].cpu().numpy(), status)
    return pat, info, st


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_solve_bitwise_on_the_block_sparse_matrix(dt):
    rows, cols, values, A, n = R.bs_case()
    b = np.random.default_rng(2).uniform(-1, 1, (n, 3))
    b[:, 1] = 0.0
    pat, info, st = _check_solve(n, rows, cols, values, b, R.BS_SIZES, dt, 200)
    assert st["stop"].tolist() == [R.CONVERGED, R.ZERO_RHS, R.CONVERGED]
    # batched: every member is bitwise the single solve
    tdt, npdt, tol = DT[dt]
    rng = np.random.default_rng(11)
    vals = np.stack([values, values * rng.uniform(0.999, 1.001, len(values)), values])
    bb = np.stack([b, rng.uniform(-1, 1, b.shape), b[:, ::-1].copy()])
    kw = dict(precond="fsai", tol=tol, max_steps=200, return_info=True)
    xb, ib = S.solve_cg(pat, _dev(vals, tdt), _dev(bb, tdt), **kw)
    for m in range(3):
        x1, i1 = S.solve_cg(pat, _dev(vals[m], tdt), _dev(bb[m], tdt), check_every=None if m else 1, **kw)
        assert _bits(xb[m]) == _bits(x1) and _bits(ib["state"][m]) == _bits(i1["state"])
        assert _bits(ib["precond_status"][m]) == _bits(i1["precond_status"])
    with pytest.raises(ValueError, match=r"precond.*'fsai'"):
        S.solve_cg(pat, _dev(values, tdt), _dev(b, tdt), precond="ilu")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_solve_bitwise_on_the_ill_conditioned_grid(dt):
    n, rows, cols, values, sizes = F.grid12()
    b = np.random.default_rng(1).uniform(-1, 1, n)
    pat, info, st = _check_solve(n, rows, cols, values, b, sizes, dt, 1000)
    if dt == "f64":  # strictly fewer iterations than block-Jacobi on the device too (at tol 1e-8; measured: 68 against 141)
        tdt, _, tol = DT[dt]
        _, ib = S.solve_cg(pat, _dev(values, tdt), _dev(b, tdt), precond="block_jacobi", tol=tol, max_steps=1000,
                           return_info=True)
        print("grid12 on the device: fsai", int(info["iterations"]), "block_jacobi", int(ib["iterations"]))
        assert int(info["stop"]) == R.CONVERGED and int(ib["stop"]) == R.CONVERGED
        assert int(info["iterations"]) < int(ib["iterations"])


# ---- frozen columns -----------------------------------------------------------------------------------------
def test_frozen_columns_beside_a_live_one():
    """scalar 0 is coupled to nothing, so the column b = e_0 converges in one iteration; column 0 is a zero
    right-hand side; column 2 runs on.  After 10 more queued iterations the stopped columns' z, x, r, p and
    records are bitwise what they were"""
    n = 300
    d = np.arange(1, n, dtype=np.int64)
    rows, cols = np.concatenate([[0], d, d[1:]]), np.concatenate([[0], d, d[:-1]])
    values = np.concatenate([[2.0], 2.0 + np.linspace(0, 1, n - 1), np.full(n - 2, -1.0)])
    b = np.zeros((n, 3))
    b[0, 1] = 3.0
    b[:, 2] = np.random.default_rng(3).uniform(-1, 1, n)
    pat = S.SymmetricPattern(rows, cols, n)
    vd, bd = _dev(values, torch.float64), _dev(b, torch.float64)
    pc = CG.Preconditioner(pat.product, "fsai", vd)
    run = CG.CgRun(pat.solver, bd, torch.zeros_like(bd), bd.clone(), lambda p, ap: pat.product.mv(vd, p, out=ap), pc,
                   1e-12, 100)
    run.start()
    for _ in range(2):
        run.iterate()
    assert run.stop().tolist() == [R.ZERO_RHS, R.CONVERGED, R.RUNNING] and run.iterations().tolist()[:2] == [0, 1]
    keep = [t.clone() for t in (run.z, run.x, run.r, run.p, run.state)]
    run.t.fill_(float("nan"))  # t is scratch: what it holds for a stopped column does not matter
    for _ in range(10):
        run.iterate()
    torch.cuda.synchronize()
    for was, now in zip(keep, (run.z, run.x, run.r, run.p, run.state)):
        for j in (0, 1):
            sel = (lambda a: a[j]) if was.dtype == torch.int64 else (lambda a: a[:, j])
            assert _bits(sel(was)) == _bits(sel(now))
    assert run.iterations().tolist()[2] == 12 and _bits(keep[1][:, 2]) != _bits(run.x[:, 2])
    assert bool(torch.isfinite(run.x).all()) and bool(torch.isfinite(run.z).all())


# ---- a bad pivot ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_bad_pivot_is_zeroed_and_reported(dt):
    tdt, npdt, tol = DT[dt]
    rows, cols, values, _, n = R.bs_case()
    v = values.copy()
    scalar = 7
    v[int(np.nonzero((rows == scalar) & (cols == scalar))[0][0])] = -5.0  # every local system with scalar 7 is indefinite
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=R.BS_SIZES)
    pl = F.plan(n, rows, cols)
    G, status = F.build(pl, v, npdt)
    pc = CG.Preconditioner(pat.product, "fsai", _dev(v, tdt))
    got = pc.values.cpu().numpy()
    assert np.isfinite(got).all() and _bits(got) == _bits(G)
    assert pc.status.tolist() == status.tolist() and status[0] == scalar and status[1] >= 1
    rs = pl["row_start"]
    zero_rows = [i for i in range(n) if not got[rs[i]:rs[i + 1]].any()]
    assert len(zero_rows) == status[1] and all(scalar in pl["cols"][rs[i]:rs[i + 1]] for i in zero_rows)
    b = np.ones((n, 2))
    x, info = S.solve_cg(pat, _dev(v, tdt), _dev(b, tdt), precond="fsai", tol=tol, max_steps=400, return_info=True)
    want, st, _ = F.entries_model(n, rows, cols, v, b, npdt, tol=tol, max_steps=400)
    assert _bits(x) == _bits(want) and bool(torch.isfinite(x).all())
    assert info["precond_status"].tolist() == status.tolist()
    assert set(info["stop"].tolist()) <= {R.CONVERGED, R.BREAKDOWN}, info["stop"]
    rec = CG.read_state(info["state"])
    assert all(np.isfinite([r[k] for k in ("rz", "pAp", "rr", "alpha", "beta")]).all() for r in rec)


# ---- gradients --------------------------------------------------------------------------------------------------
def test_gradients_against_solve():
    rows, cols, values, A, n = R.bs_case()
    kappa = float(np.linalg.cond(A))
    tol = 1e-12
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=R.BS_SIZES)
    rng = np.random.default_rng(6)
    b, w = rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2))
    wd = _dev(w, torch.float64)
    grads = []
    for fn in (lambda v, bb: S.solve(pat, v, bb),
               lambda v, bb: S.solve_cg(pat, v, bb, precond="fsai", tol=tol, max_steps=400)):
        v = _dev(values, torch.float64).requires_grad_(True)
        bb = _dev(b, torch.float64).requires_grad_(True)
        (fn(v, bb) * wd).sum().backward()
        grads.append((v.grad.cpu().numpy(), bb.grad.cpu().numpy()))
    for got, want, name in zip(grads[1], grads[0], ("values", "b")):
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print("gradient of", name, "relative difference", rel, "bound", 100 * kappa * tol)
        assert rel <= 100 * kappa * tol, (name, rel)


# ---- call history ---------------------------------------------------------------------------------------------
def test_a_used_product_gives_the_bits_of_a_fresh_one():
    rows, cols, values, _, n = R.bs_case()
    b = np.random.default_rng(4).uniform(-1, 1, (n, 2))
    fresh = S.SymmetricPattern(rows, cols, n, param_sizes=R.BS_SIZES)
    used = S.SymmetricPattern(rows, cols, n, param_sizes=R.BS_SIZES)
    for k, kind in enumerate(("jacobi", "block_jacobi", "jacobi", "block_jacobi")):
        tdt = (torch.float32, torch.float64)[k % 2] if k < 2 else (torch.float64, torch.float32)[k % 2]
        S.solve_cg(used, _dev(values, tdt), _dev(b, tdt), precond=kind, max_steps=3)
    for dt in ("f32", "f64", "f32"):
        tdt, _, tol = DT[dt]
        kw = dict(precond="fsai", tol=tol, max_steps=200, return_info=True)
        xu, iu = S.solve_cg(used, _dev(values, tdt), _dev(b, tdt), **kw)
        xf, jf = S.solve_cg(fresh, _dev(values, tdt), _dev(b, tdt), **kw)
        assert _bits(xu) == _bits(xf) and _bits(iu["state"]) == _bits(jf["state"])
        assert _bits(iu["precond_status"]) == _bits(jf["precond_status"])
        S.solve_cg(used, _dev(values, tdt), _dev(b, tdt), precond="block_jacobi", max_steps=2)


# ---- buffers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,q", [("hub65", 3), (1025, 1)])
def test_entries_on_framed_poisoned_offset_buffers(name, q, dt):
    tdt, npdt, _ = DT[dt]
    n, rows, cols, tri, values, pat, pl = _case(name)
    sol, prod, lib = pat.solver, pat.product, pat.product._lib
    sfx = "f64" if dt == "f64" else "f32"
    i64, P = ctypes.c_int64, ctypes.c_void_p
    err = lambda: lib.bsp_last_error().decode()
    elems, nnz = int(pl["row_start"][-1]), len(rows)
    r = np.random.default_rng(5).uniform(-1, 1, (n, q)).astype(npdt)
    # payloads: 0 values, 1 G, 2 r, 3 t, 4 z: each at an odd element offset between guards of the sentinel
    fr = BE.Frame([nnz, elems, n * q, n * q, n * q], npdt)
    fr.fill(0, values[0].astype(npdt)).fill(2, r).seal()
    need = i64(0)
    assert lib.bsp_cg_work_bytes(sol._h, i64(n), i64(q), ctypes.byref(need)) == 0
    work = BE.Frame([need.value // 8], np.float64, align_bytes=16)  # exactly the documented size, 16-byte aligned
    status = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    state = torch.zeros((q, 12), dtype=torch.int64, device="cuda")
    ptr = lambda k: P(fr.view(k).data_ptr())
    wp, sp = P(work.view(0).data_ptr()), P(state.data_ptr())
    assert all(fr.view(k).data_ptr() % 16 != 0 for k in range(5))
    build = getattr(lib, "bsp_cg_precond_build_" + sfx)
    apply = getattr(lib, "bsp_fsai_apply_" + sfx)
    init = getattr(lib, "bsp_cg_init_" + sfx)
    # refusals come before any device work: the frames still hold what they held
    assert build(sol._h, prod._h, ctypes.c_int32(3), ptr(0), ptr(0), wp, P(status.data_ptr())) != 0 and "aliases" in err()
    assert apply(sol._h, prod._h, i64(n), i64(q), ptr(1), ptr(2), ptr(3), ptr(3), wp, sp) != 0 and "aliases" in err()
    assert apply(sol._h, prod._h, i64(n), i64(q), ptr(1), ptr(2), ptr(2), ptr(4), wp, sp) != 0 and "aliases" in err()
    assert apply(sol._h, prod._h, i64(n), i64(q), ptr(1), ptr(2), ptr(3), ptr(4), P(wp.value + 8), sp) != 0
    assert "16-byte aligned" in err()
    torch.cuda.synchronize()
    fr.assert_intact(read_only=(0, 2), what="refusals")
    assert BE.is_sentinel(fr.host(1)).all() and BE.is_sentinel(fr.host(3)).all() and BE.is_sentinel(fr.host(4)).all()
    assert status.tolist() == [-7, -7]
    # the build, then the records of a solve from x = 0 (r = b), then the apply
    assert build(sol._h, prod._h, ctypes.c_int32(3), ptr(0), ptr(1), wp, P(status.data_ptr())) == 0, err()
    x = torch.zeros((n, q), dtype=tdt, device="cuda")
    bd = _dev(r, tdt)
    assert init(sol._h, i64(n), i64(q), P(bd.data_ptr()), P(x.data_ptr()), ptr(2), ctypes.c_double(1e-10), i64(5),
                ctypes.c_int32(0), wp, sp) == 0, err()
    fr.seal()
    assert apply(sol._h, prod._h, i64(n), i64(q), ptr(1), ptr(2), ptr(3), ptr(4), wp, sp) == 0, err()
    torch.cuda.synchronize()
    fr.assert_intact(read_only=(0, 1, 2), what="build and apply")
    work.assert_intact(what="the work area")
    G, st = F.build(pl, values[0], npdt)
    t, z = F.apply(pl, G, r)
    assert _bits(fr.host(1)) == _bits(G) and status.tolist() == st.tolist()
    assert _bits(fr.host(3)) == _bits(t) and _bits(fr.host(4)) == _bits(z)
    rz = R.dot(r, z)
    for j, rec in enumerate(CG.read_state(state)):
        assert np.float64(rec["rz"]).tobytes() == np.float64(rz[j]).tobytes() and rec["stop"] == R.RUNNING
