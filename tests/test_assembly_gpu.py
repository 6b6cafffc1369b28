"""GPU: the coordinate-entry assembly on the MI355X.  assemble must be bitwise
np.add.at(zeros(dataSize), entryOffsets, values) (duplicates, shuffled order, a run of more than 10 000
entries, an output full of NaN); the adjoint bitwise grad_data[entryOffsets]; batch members bitwise
the single call, across the 65535 chunk limit; baspacho_amd.sparse must match dense torch in value
and gradient, pass gradcheck, run on any stream without host syncs, and refuse bad arguments before
device work."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import sparse as S
from assembly_ref import dense_user, duplicated, stored_elements
from helpers import solver_random
from selinv_cases import build_case

pytestmark = pytest.mark.gpu

DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}


def _cases():
    return {"random_elim": lambda: solver_random(71, size=18, fill=0.12, elim=(0, 8), ranges=[0, 8])[0],
            "random_wide": lambda: solver_random(73, size=60, fill=0.1, pmin=1, pmax=7)[0],
            "small/n3_r170": lambda: build_case("small/n3_r170")[0],
            "width17": lambda: build_case("width17")[0]}


def _np_assemble(sol, offs, values, npdt):
    out = np.zeros(sol.dataSize(), dtype=npdt)
    keep = offs >= 0
    np.add.at(out, offs[keep], values[keep].astype(npdt))
    return out


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("triangle", ["lower", "full"])
@pytest.mark.parametrize("case", list(_cases()))
def test_assemble_bitwise(case, triangle, dt):
    tdt, npdt = DT[dt]
    sol = _cases()[case]()
    rng = np.random.default_rng(11)
    rows, cols, values = duplicated(*stored_elements(sol), rng, full=(triangle == "full"))
    asm = sol.assembly(rows, cols, triangle)
    offs = asm.entryOffsets()
    out = torch.full((sol.dataSize(),), float("nan"), dtype=tdt, device="cuda")
    got = asm.assemble(torch.from_numpy(values.astype(npdt)).cuda(), out=out)
    assert got is out
    got = got.cpu().numpy()
    assert _bits_equal(got, _np_assemble(sol, offs, values, npdt))
    sp = sol.scalarPermutation()
    dense = sol.densify(got.astype(np.float64), fill_upper_half=True)[np.ix_(sp, sp)]
    ref = dense_user(sol.order(), rows, cols, values.astype(npdt).astype(np.float64))
    np.testing.assert_allclose(dense, ref, rtol=1e-5 if dt == "f32" else 1e-13, atol=1e-5 if dt == "f32" else 1e-13)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_assemble_long_runs(dt):
    tdt, npdt = DT[dt]
    sol = _cases()["random_wide"]()
    r0, c0 = stored_elements(sol)
    rng = np.random.default_rng(3)
    # 12 345 contributions on one element, 65 / 64 / 200 on three others, 1..8 on the rest, shuffled
    extra = [(0, 12345), (1, 65), (2, 64), (5, 200)]
    rows = np.concatenate([r0] + [np.full(m, r0[e]) for e, m in extra])
    cols = np.concatenate([c0] + [np.full(m, c0[e]) for e, m in extra])
    rows, cols, values = duplicated(rows, cols, rng)
    asm = sol.assembly(rows, cols)
    assert asm.info()["max_run"] > 10000 and asm.info()["long_runs"] >= 3
    out = torch.full((sol.dataSize(),), float("nan"), dtype=tdt, device="cuda")
    asm.assemble(torch.from_numpy(values.astype(npdt)).cuda(), out=out)
    assert _bits_equal(out.cpu().numpy(), _np_assemble(sol, asm.entryOffsets(), values, npdt))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_adjoint_bitwise(dt):
    tdt, npdt = DT[dt]
    sol = _cases()["random_elim"]()
    rows, cols, _ = duplicated(*stored_elements(sol), np.random.default_rng(4), full=True)
    asm = sol.assembly(rows, cols, "full")
    offs = asm.entryOffsets()
    gd = np.random.default_rng(5).uniform(-1, 1, sol.dataSize()).astype(npdt)
    out = torch.full((len(rows),), float("nan"), dtype=tdt, device="cuda")
    asm.adjoint(torch.from_numpy(gd).cuda(), out=out)
    assert _bits_equal(out.cpu().numpy(), np.where(offs >= 0, gd[np.maximum(offs, 0)], npdt(0)))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_batch_members_bitwise(dt):
    tdt, npdt = DT[dt]
    sol = _cases()["small/n3_r170"]()
    rows, cols, _ = duplicated(*stored_elements(sol), np.random.default_rng(6))
    asm = sol.assembly(rows, cols)
    vals = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (5, len(rows))).astype(npdt)).cuda()
    data = torch.full((5, sol.dataSize()), float("nan"), dtype=tdt, device="cuda")
    asm.assemble(vals, out=data)
    gv = asm.adjoint(data)
    for q in range(5):
        one = asm.assemble(vals[q].clone())
        assert torch.equal(one, data[q])
        assert _bits_equal(data[q].cpu().numpy(), _np_assemble(sol, asm.entryOffsets(), vals[q].cpu().numpy(), npdt))
        assert torch.equal(asm.adjoint(data[q].clone()), gv[q])


def test_batch_past_chunk_limit():
    sol = solver_random(74, size=4, fill=0.5, pmin=1, pmax=2)[0]
    r0, c0 = stored_elements(sol)
    asm = sol.assembly(r0, c0)
    offs = asm.entryOffsets()
    batch = 70000
    vals = torch.rand(batch, len(r0), dtype=torch.float32, device="cuda")
    data = torch.full((batch, sol.dataSize()), float("nan"), dtype=torch.float32, device="cuda")
    asm.assemble(vals, out=data)
    expect = torch.zeros_like(data)
    expect[:, torch.from_numpy(offs).cuda()] = vals
    assert torch.equal(data, expect)
    gv = asm.adjoint(data)
    assert torch.equal(gv, vals)
    for q in (0, 65534, 65535, batch - 1):
        assert torch.equal(asm.assemble(vals[q].clone()), data[q])


def test_nnz_zero_writes_zeros():
    sol = _cases()["random_elim"]()
    asm = sol.assembly([], [])
    out = torch.full((sol.dataSize(),), float("nan"), dtype=torch.float64, device="cuda")
    asm.assemble(torch.zeros(0, dtype=torch.float64, device="cuda"), out=out)
    assert torch.equal(out, torch.zeros_like(out))
    assert asm.adjoint(out).shape == (0,)


# ---- baspacho_amd.sparse -----------------------------------------------------------------------
def _spd_entries(n, rng, dup=3, triangle="lower", density=0.15):
    """entries of a diagonally dominant SPD matrix, every value split into 1..dup contributions"""
    i, j = np.nonzero(np.tril(rng.random((n, n)) < density, -1))
    rows = np.concatenate([i, np.arange(n)])
    cols = np.concatenate([j, np.arange(n)])
    rows, cols, _ = duplicated(rows, cols, rng, max_dup=dup, full=(triangle == "full"))
    values = np.where(rows == cols, rng.uniform(1.0, 2.0, len(rows)) * n / 2, rng.uniform(-1, 1, len(rows)))
    return rows, cols, values


def _dense_torch(n, rows, cols, values):
    """differentiable dense A of the entries (lower triangle summed, mirrored)"""
    keep = torch.from_numpy(rows >= cols).to(values.device)
    r = torch.from_numpy(rows).to(values.device)[keep]
    c = torch.from_numpy(cols).to(values.device)[keep]
    L = torch.zeros(n, n, dtype=values.dtype, device=values.device).index_put((r, c), values[keep], accumulate=True)
    return torch.tril(L) + torch.tril(L, -1).T


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("sizes", [None, "blocks"])
def test_sparse_solve_logdet_match_dense(dt, sizes):
    tdt, _ = DT[dt]
    rng = np.random.default_rng(8)
    n = 40
    ps = None if sizes is None else [3, 1, 2, 4, 2, 3, 1, 5, 2, 3, 2, 4, 1, 3, 2, 2]
    rows, cols, values = _spd_entries(n, rng)
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=ps)
    v = torch.from_numpy(values).to("cuda", tdt)
    b = torch.randn(n, 3, dtype=tdt, device="cuda")
    A = _dense_torch(n, rows, cols, v).double()
    x = S.solve(pat, v, b)
    ld = S.logdet(pat, v)
    x2, ld2 = S.solve_logdet(pat, v, b[:, 0])
    tol = dict(rtol=1e-4, atol=1e-4) if dt == "f32" else dict(rtol=1e-10, atol=1e-10)
    Lc = torch.linalg.cholesky(A)
    torch.testing.assert_close(x.double(), torch.cholesky_solve(b.double(), Lc), **tol)
    torch.testing.assert_close(x2.double(), torch.cholesky_solve(b[:, :1].double(), Lc)[:, 0], **tol)
    torch.testing.assert_close(ld.double(), torch.logdet(A), **tol)
    torch.testing.assert_close(ld2.double(), torch.logdet(A), **tol)


@pytest.mark.parametrize("triangle", ["lower", "full"])
def test_sparse_gradcheck(triangle):
    rng = np.random.default_rng(9)
    n = 9
    rows, cols, values = _spd_entries(n, rng, dup=3, triangle=triangle, density=0.3)
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=[2, 1, 3, 1, 2], triangle=triangle)
    v = torch.from_numpy(values).cuda().requires_grad_()
    b = torch.randn(n, 2, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda v_, b_: S.solve(pat, v_, b_), (v, b))
    assert torch.autograd.gradcheck(lambda v_: S.logdet(pat, v_), (v,))
    assert torch.autograd.gradcheck(lambda v_, b_: S.solve_logdet(pat, v_, b_), (v, b))
    assert torch.autograd.gradcheck(lambda v_: S.assemble(pat, v_), (v,))


@pytest.mark.parametrize("triangle", ["lower", "full"])
def test_sparse_grads_match_dense_autograd(triangle):
    rng = np.random.default_rng(10)
    n = 30
    rows, cols, values = _spd_entries(n, rng, triangle=triangle)
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=[2] * 15, triangle=triangle)
    w = torch.randn(n, 2, dtype=torch.float64, device="cuda")
    v1 = torch.from_numpy(values).cuda().requires_grad_()
    b1 = torch.randn(n, 2, dtype=torch.float64, device="cuda", requires_grad=True)
    x, ld = S.solve_logdet(pat, v1, b1)
    ((x * w).sum() + 0.7 * ld).backward()
    v2 = v1.detach().clone().requires_grad_()
    b2 = b1.detach().clone().requires_grad_()
    A = _dense_torch(n, rows, cols, v2)
    ((torch.linalg.solve(A, b2) * w).sum() + 0.7 * torch.logdet(A)).backward()
    torch.testing.assert_close(v1.grad, v2.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(b1.grad, b2.grad, rtol=1e-10, atol=1e-10)
    if triangle == "full":
        assert torch.all(v1.grad[torch.from_numpy(rows < cols).cuda()] == 0)


def test_sparse_batched_matches_single():
    rng = np.random.default_rng(12)
    n = 25
    rows, cols, values = _spd_entries(n, rng)
    pat = S.SymmetricPattern(rows, cols, n)
    vb = torch.from_numpy(np.stack([values, values * 1.5, values * 0.75])).cuda()
    bb = torch.randn(3, n, dtype=torch.float64, device="cuda")
    xb, ldb = S.solve_logdet(pat, vb, bb)
    for q in range(3):
        x, ld = S.solve_logdet(pat, vb[q].contiguous(), bb[q])
        torch.testing.assert_close(xb[q], x, rtol=0, atol=0)
        torch.testing.assert_close(ldb[q], ld, rtol=0, atol=0)


def test_sparse_from_torch():
    rng = np.random.default_rng(13)
    n = 20
    rows, cols, values = _spd_entries(n, rng, triangle="full")
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, cols])), torch.from_numpy(values), (n, n))
    pat, v = S.SymmetricPattern.from_torch(A, triangle="full")
    ld = S.logdet(pat, v.cuda())
    torch.testing.assert_close(ld.cpu(), torch.logdet(_dense_torch(n, rows, cols, torch.from_numpy(values))),
                               rtol=1e-10, atol=1e-10)
    Ac = _dense_torch(n, rows, cols, torch.from_numpy(values))
    pat2, v2 = S.SymmetricPattern.from_torch(torch.tril(Ac).to_sparse_csr())
    b = torch.randn(n, dtype=torch.float64)
    x = S.solve(pat2, v2.cuda(), b.cuda())
    torch.testing.assert_close(x.cpu(), torch.linalg.solve(Ac, b), rtol=1e-10, atol=1e-10)


def test_sparse_on_side_stream():
    rng = np.random.default_rng(14)
    n = 30
    rows, cols, values = _spd_entries(n, rng)
    pat = S.SymmetricPattern(rows, cols, n)
    v = torch.from_numpy(values).cuda().requires_grad_()
    b = torch.randn(n, dtype=torch.float64, device="cuda")
    x0, ld0 = S.solve_logdet(pat, v, b)
    (x0.sum() + ld0).backward()
    g0 = v.grad.clone()
    v.grad = None
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x1, ld1 = S.solve_logdet(pat, v, b)
        (x1.sum() + ld1).backward()
    torch.cuda.current_stream().wait_stream(s)
    assert pat.solver._stream is None
    torch.testing.assert_close(x1, x0, rtol=0, atol=0)
    torch.testing.assert_close(ld1, ld0, rtol=0, atol=0)
    torch.testing.assert_close(v.grad, g0, rtol=0, atol=0)


def test_sparse_no_host_sync():
    rng = np.random.default_rng(15)
    n = 30
    rows, cols, values = _spd_entries(n, rng)
    pat = S.SymmetricPattern(rows, cols, n)
    v = torch.from_numpy(values).cuda().requires_grad_()
    b = torch.randn(n, 2, dtype=torch.float64, device="cuda", requires_grad=True)
    x, ld = S.solve_logdet(pat, v, b)  # first call: uploads the map and the permutation
    (x.sum() + ld).backward()
    v.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, ld = S.solve_logdet(pat, v, b)
        (x.sum() + ld).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(v.grad).all() and torch.isfinite(b.grad).all()


def test_argument_errors_before_device_work():
    sol = _cases()["random_elim"]()
    other = _cases()["random_elim"]()
    r0, c0 = stored_elements(sol)
    asm = sol.assembly(r0, c0)
    lib = sol._lib
    vals = torch.rand(len(r0), dtype=torch.float64, device="cuda")
    out = torch.full((2, sol.dataSize()), float("nan"), dtype=torch.float64, device="cuda")
    vp, o0, o1 = vals.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    P = ctypes.c_void_p

    def err(rc):
        assert rc != 0
        return lib.bsp_last_error().decode()

    assert "another solver" in err(lib.bsp_assemble_f64(other._h, asm._h, P(vp), P(o0)))
    assert "values pointer of batch member 0 is NULL" in err(lib.bsp_assemble_f64(sol._h, asm._h, P(None), P(o0)))
    assert "data pointer of batch member 0 is NULL" in err(lib.bsp_assemble_f64(sol._h, asm._h, P(vp), P(None)))
    arr = lambda *p: (P * len(p))(*p)
    assert "batch is empty" in err(lib.bsp_assemble_batched_f64(sol._h, asm._h, arr(vp), arr(o0), 0))
    assert "NULL" in err(lib.bsp_assemble_batched_f64(sol._h, asm._h, None, arr(o0), 1))
    assert "repeats" in err(lib.bsp_assemble_batched_f64(sol._h, asm._h, arr(vp, vp), arr(o0, o0), 2))
    assert "batch member 1 is NULL" in err(lib.bsp_assemble_batched_f64(sol._h, asm._h, arr(vp, None), arr(o0, o1), 2))
    assert "another solver" in err(lib.bsp_assemble_adjoint_batched_f64(other._h, asm._h, arr(o0), arr(vp), 1))
    assert "repeats" in err(lib.bsp_assemble_adjoint_batched_f64(sol._h, asm._h, arr(o0, o1), arr(vp, vp), 2))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # nothing was written
    with pytest.raises(ValueError):
        asm.assemble(vals[:-1])
    with pytest.raises(ValueError):
        asm.assemble(vals, out=out)
    with pytest.raises(TypeError):
        asm.assemble(vals.to(torch.int64))
    pat = S.SymmetricPattern([0, 1, 1], [0, 0, 1], 2)
    with pytest.raises(ValueError, match="n = 2"):
        S.solve(pat, torch.tensor([4.0, 1.0, 4.0], dtype=torch.float64, device="cuda"),
                torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="device memory"):
        S.logdet(pat, torch.tensor([4.0, 1.0, 4.0], dtype=torch.float64))
