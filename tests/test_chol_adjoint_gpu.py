"""GPU: Solver.factorAdjoint (the reverse-mode sweep of factor(), hip_chol_adjoint_kernels.h) and
Solver.patternOuter against the dense references of chol_adjoint_ref.py and autograd_ref.py.

Data: known-factor matrices A = L0 L0^T (known_factor.py, rho = 0.5), whose condition numbers are
below 10 on these skeletons (asserted).  With cond(A) < 100 the expected error of the gradient is of
order cond(A) eps times a modest growth factor; the bounds below are set from that before any GPU
run: 1e-10 in fp64 and 1e-4 in fp32, relative to max |grad|.  fp32 runs are compared with the
oracle of the fp32-rounded data."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import testing as T
from autograd_ref import element_coords, pattern_grad_ref
from chol_adjoint_ref import dense_grad, lbar_random, rel_error
from helpers import solver_random, spd_data, to_dev
from known_factor import known_factor_data
from selinv_cases import build_case, case_names

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}
TDT = {np.float64: torch.float64, np.float32: torch.float32}


def _data(sol, seed, dtype):
    kf = known_factor_data(sol, seed, dtype, rho=0.5)
    assert np.linalg.cond(kf.A) < 100
    return kf.data


def _factor(sol, data):
    L = to_dev(data)
    sol.factor(L)
    return L


def _adjoint(sol, L, lbar):
    g = lbar.clone()
    sol.factorAdjoint(L, g)
    return g


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", case_names())
def test_selinv_cases_against_dense_oracle(name, dtype):
    sol, expect = build_case(name)
    expect(sol._testSelInvPlan())
    data = _data(sol, 5, dtype)
    lbar = lbar_random(sol, 11, dtype)
    L = _factor(sol, data)
    L0 = L.clone()
    g = _adjoint(sol, L, to_dev(lbar))
    g2 = _adjoint(sol, L, to_dev(lbar))
    torch.cuda.synchronize()
    assert torch.equal(L, L0), "factorAdjoint wrote to L"
    assert torch.equal(g, g2), "two runs differ"
    got = g.cpu().numpy()
    want = dense_grad(sol, data, lbar)
    err = rel_error(got, want)
    assert np.isfinite(got).all() and err < TOL[dtype], (name, err)
    i, j = element_coords(sol)
    assert (got[i < j] == 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed", [3, 8])
def test_random_structures_with_elimination_ranges(seed, dtype):
    sol, _, _ = solver_random(seed, fill=0.037, elim=(0, 60))
    assert len(sol.sparseEliminationRanges()) >= 2
    data = _data(sol, seed, dtype)
    lbar = lbar_random(sol, seed + 1, dtype)
    g = _adjoint(sol, _factor(sol, data), to_dev(lbar))
    err = rel_error(g.cpu().numpy(), dense_grad(sol, data, lbar))
    assert err < TOL[dtype], err


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_members_are_bitwise_the_single_call(dtype):
    sol, _ = build_case("mixed_owners")
    data = _data(sol, 2, dtype)
    L = _factor(sol, data)
    for B_ in (1, 2, 5, 17):
        lbars = [to_dev(lbar_random(sol, 100 + q, dtype)) for q in range(B_)]
        Ls = [L.clone() for _ in range(B_)]
        single = [_adjoint(sol, L, lb) for lb in lbars]
        gs = [lb.clone() for lb in lbars]
        sol.factorAdjoint(Ls, gs)
        torch.cuda.synchronize()
        for q in range(B_):
            assert torch.equal(gs[q], single[q]), (B_, q)
            assert torch.equal(Ls[q], L)


def test_batch_in_chunks_is_bitwise_the_single_call():
    sol, _ = build_case("width129")
    data = _data(sol, 4, np.float64)
    L = _factor(sol, data)
    lbars = [to_dev(lbar_random(sol, 7 + q)) for q in range(5)]
    single = [_adjoint(sol, L, lb) for lb in lbars]
    sol._testSetSelInvBatchChunk(2)
    try:
        gs = [lb.clone() for lb in lbars]
        sol.factorAdjoint([L] * 5, gs)  # one factor read by every member
    finally:
        sol._testSetSelInvBatchChunk(0)
    torch.cuda.synchronize()
    for q in range(5):
        assert torch.equal(gs[q], single[q]), q


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_log_determinant_gradient_from_diag_lbar(dtype):
    """Lbar = diag(2 / L_ii) is the factor's share of log det A: the result is patternGrad(Z) with Z
    the selected inverse"""
    sol, _ = build_case("forest")
    data = _data(sol, 6, dtype)
    L = _factor(sol, data)
    i, j = element_coords(sol)
    diag = torch.as_tensor(np.nonzero(i == j)[0], device="cuda")
    lbar = torch.zeros_like(L)
    lbar[diag] = 2.0 / L[diag]
    g = _adjoint(sol, L, lbar)
    Z = L.clone()
    sol.selectedInverse(Z)
    want = torch.empty_like(L)
    one = torch.ones(1, dtype=L.dtype, device="cuda")
    sol.patternGrad(want, Z=Z, zScale=one)
    err = rel_error(g.cpu().numpy(), want.cpu().numpy())
    assert err < TOL[dtype], err


@pytest.mark.parametrize("which", ["grid82", "meri"])
def test_full_size_finite_difference(which):
    if which == "grid82":
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
    else:
        ss = T.gen_meridians(4, 1500, 0.5, 120, 600, 2, 2, 37)
    sol = B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)
    data = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
    sol.damp(data, 0.0, sol.order() * 1.2)
    low = torch.as_tensor(sol.lowerMask(), device="cuda")
    rng = np.random.default_rng(5)
    W = to_dev(rng.uniform(-1, 1, sol.dataSize())) * low
    dirn = to_dev(rng.uniform(-1, 1, sol.dataSize())) * low
    d0 = to_dev(data)

    def f(d):
        L = d.clone()
        sol.factor(L)
        return L, float(torch.dot(W, L * low))

    L, _ = f(d0)
    g = _adjoint(sol, L, W)
    h = 1e-4
    fd = (f(d0 + h * dirn)[1] - f(d0 - h * dirn)[1]) / (2 * h)
    an = float(torch.dot(g, dirn))
    scale = float(torch.dot(g.abs(), dirn.abs()))
    assert abs(fd - an) < 1e-6 * scale, (fd, an, scale)


# ---- patternOuter ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_pattern_outer_against_numpy(dtype, k):
    sol, _, _ = solver_random(3, fill=0.037, elim=(0, 60))
    n = sol.order()
    rng = np.random.default_rng(k)
    U, V = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    i, j = element_coords(sol)
    want = np.where(i >= j, -0.5 * np.einsum("ek,ek->e", U[i], V[j]), 0.0)
    out = torch.full((sol.dataSize(),), 7.0, dtype=TDT[dtype], device="cuda")
    sol.patternOuter(out, to_dev(U.T.astype(dtype)), to_dev(V.T.astype(dtype)), nRHS=k, alpha=-0.5)
    err = rel_error(out.cpu().numpy(), want)
    assert err < (1e-14 if dtype == np.float64 else 1e-6), err
    # batch: member q bitwise the single call
    outs = [torch.empty_like(out) for _ in range(3)]
    Us = [to_dev((U.T * (q + 1)).astype(dtype)) for q in range(3)]
    Vs = [to_dev(V.T.astype(dtype)) for _ in range(3)]
    sol.patternOuter(outs, Us, Vs, nRHS=k, alpha=-0.5)
    for q in range(3):
        one = torch.empty_like(out)
        sol.patternOuter(one, Us[q], Vs[q], nRHS=k, alpha=-0.5)
        assert torch.equal(one, outs[q])


def test_pattern_grad_unchanged_beside_outer():
    """the symmetric projection keeps its result (its entry points and instantiation are untouched)"""
    sol, _, _ = solver_random(8, fill=0.037, elim=(0, 60))
    n = sol.order()
    rng = np.random.default_rng(2)
    U, V = rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2))
    out = torch.empty(sol.dataSize(), dtype=torch.float64, device="cuda")
    sol.patternGrad(out, U=to_dev(U.T), V=to_dev(V.T), nRHS=2, alpha=1.0)
    assert rel_error(out.cpu().numpy(), pattern_grad_ref(sol, U=U, V=V)) < 1e-14


# ---- refusals ------------------------------------------------------------------------------------
def _rc(fn, *args):
    rc = fn(*args)
    return rc, B._lib.load().bsp_last_error().decode()


def test_factor_adjoint_refusals():
    sol, _ = build_case("mixed_owners")
    lib, h = sol._lib, sol._h
    ds = sol.dataSize()
    L = torch.ones(ds, dtype=torch.float64, device="cuda")
    g = torch.zeros(3 * ds, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p
    lp, gp = L.data_ptr(), g.data_ptr()
    for fn in (lib.bsp_factor_adjoint_f64, lib.bsp_factor_adjoint_f32):
        assert _rc(fn, h, p(None), p(gp))[0] != 0
        assert _rc(fn, h, p(lp), p(None))[0] != 0
        rc, msg = _rc(fn, h, p(lp), p(lp))
        assert rc != 0 and "overlaps" in msg, msg
    arr = lambda *xs: (p * len(xs))(*[p(x) for x in xs])
    for fn in (lib.bsp_factor_adjoint_batched_f64, lib.bsp_factor_adjoint_batched_f32):
        rc, msg = _rc(fn, h, arr(lp), arr(gp), ctypes.c_int32(0))
        assert rc != 0 and "empty" in msg, msg
        assert _rc(fn, h, None, arr(gp), ctypes.c_int32(1))[0] != 0
        assert _rc(fn, h, arr(lp), None, ctypes.c_int32(1))[0] != 0
        rc, msg = _rc(fn, h, arr(lp, lp), arr(gp, None), ctypes.c_int32(2))
        assert rc != 0 and "NULL" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, lp), arr(gp, gp), ctypes.c_int32(2))
        assert rc != 0 and "overlap" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, lp), arr(gp, gp + 8), ctypes.c_int32(2))
        assert rc != 0 and "overlap" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, gp + 8 * ds), arr(gp, gp + 8 * ds), ctypes.c_int32(2))
        assert rc != 0 and "overlaps input" in msg, msg
    # the refused calls did no device work
    torch.cuda.synchronize()
    assert (g == 0).all() and (L == 1).all()
    inc, _, _ = solver_random(61, fill=0.03, elim=(0, 60), ranges=[0, 60], policy=B.AddFillForGivenElims)
    assert inc.canFactorUpToSpan() < inc.numSpans()
    d = torch.zeros(inc.dataSize(), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="complete factor"):
        inc.factorAdjoint(d, d.clone())
    with pytest.raises(RuntimeError, match="complete factor"):
        inc.patternOuter(d, torch.zeros(inc.order(), dtype=torch.float64, device="cuda"),
                         torch.zeros(inc.order(), dtype=torch.float64, device="cuda"))


def test_pattern_outer_refusals():
    sol, _ = build_case("mixed_owners")
    lib, h = sol._lib, sol._h
    ds, n = sol.dataSize(), sol.order()
    out = torch.zeros(2 * ds, dtype=torch.float64, device="cuda")
    U = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p
    op, up = out.data_ptr(), U.data_ptr()
    one = lambda v: ctypes.c_double(v)
    for fn, real in ((lib.bsp_pattern_outer_f64, ctypes.c_double), (lib.bsp_pattern_outer_f32, ctypes.c_float)):
        assert _rc(fn, h, p(None), p(up), ctypes.c_int64(n), ctypes.c_int32(1), real(1), p(op))[0] != 0
        assert _rc(fn, h, p(up), p(up), ctypes.c_int64(n), ctypes.c_int32(1), real(1), p(None))[0] != 0
        rc, msg = _rc(fn, h, p(up), p(up), ctypes.c_int64(n), ctypes.c_int32(0), real(1), p(op))
        assert rc != 0 and "nRHS" in msg, msg
        rc, msg = _rc(fn, h, p(up), p(up), ctypes.c_int64(n - 1), ctypes.c_int32(1), real(1), p(op))
        assert rc != 0 and "stride" in msg, msg
        rc, msg = _rc(fn, h, p(op), p(up), ctypes.c_int64(n), ctypes.c_int32(1), real(1), p(op))
        assert rc != 0 and "overlaps input" in msg, msg
    arr = lambda *xs: (p * len(xs))(*[p(x) for x in xs])
    for fn, real in ((lib.bsp_pattern_outer_batched_f64, ctypes.c_double),
                     (lib.bsp_pattern_outer_batched_f32, ctypes.c_float)):
        args = lambda o, b: (h, arr(up, up), arr(up, up), ctypes.c_int64(n), ctypes.c_int32(1), real(1), o,
                             ctypes.c_int32(b))
        rc, msg = _rc(fn, *args(arr(op, op + 8 * ds), 0))
        assert rc != 0 and "empty" in msg, msg
        assert _rc(fn, *args(None, 2))[0] != 0
        rc, msg = _rc(fn, *args(arr(op, op), 2))
        assert rc != 0 and "overlap" in msg, msg
        rc, msg = _rc(fn, *args(arr(op, None), 2))
        assert rc != 0 and "NULL" in msg, msg
    torch.cuda.synchronize()
    assert (out == 0).all()
