"""GPU: Solver.selectedInverseAdjoint (the reverse mode of selectedInverse(),
hip_selinv_adjoint_kernels.h) against the dense references of selinv_adjoint_ref.py.

Data: known-factor matrices A = L0 L0^T (known_factor.py, rho = 0.5) with cond(A) < 100 (asserted);
grad is uniform(-1, 1) on EVERY slot, mirrors included.  Bounds, those test_chol_adjoint_gpu.py derives
for these matrices before any GPU run: 1e-10 in fp64 and 1e-4 in fp32, relative to max |want| (the
restatement with every array in fp32 sits at 1.2e-6 on the CPU, so the fp32 bound leaves the
algorithm's own rounding about 80 x headroom).  fp32 runs are compared with the oracle of the
fp32-rounded data.

The scatter of the sweep adds with float atomics wherever a level holds more than one node, and in
every small lump: a batch member is CLOSE to the single call, not bitwise, so the batch tests check
every member against its own oracle and assert no bitwise equality."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import testing as T
from autograd_ref import element_coords
from chol_adjoint_ref import dense_factor
from helpers import solver_random, to_dev
from known_factor import known_factor_data
from selinv_adjoint_ref import dense_lbar, grad_random, rel_error, zsz_projection
from selinv_cases import build_case, case_names

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-10, np.float32: 1e-4}


def _data(sol, seed, dtype):
    kf = known_factor_data(sol, seed, dtype, rho=0.5)
    assert np.linalg.cond(kf.A) < 100
    return kf.data


def _factor_and_z(sol, data):
    L = to_dev(data)
    sol.factor(L)
    Z = L.clone()
    sol.selectedInverse(Z)
    return L, Z


def _adjoint(sol, L, Z, grad):
    g = grad.clone()
    sol.selectedInverseAdjoint(L, Z, g)
    return g


def _check_against_oracle(sol, data, grad, dtype, tag):
    L, Z = _factor_and_z(sol, data)
    L0, Z0 = L.clone(), Z.clone()
    g = _adjoint(sol, L, Z, to_dev(grad))
    torch.cuda.synchronize()
    assert torch.equal(L, L0) and torch.equal(Z, Z0), "selectedInverseAdjoint wrote to L or Z"
    got = g.cpu().numpy()
    coords = element_coords(sol)
    want = dense_lbar(sol, dense_factor(sol, data), grad, coords)
    err = rel_error(got, want)
    print("%s %s: rel. error %.3e" % (tag, np.dtype(dtype).name, err))
    assert np.isfinite(got).all() and err < TOL[dtype], (tag, err)
    i, j = coords
    assert (got[i < j] == 0).all()
    return L, g


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", case_names())
def test_selinv_cases_against_dense_oracle(name, dtype):
    sol, expect = build_case(name)
    expect(sol._testSelInvPlan())
    _check_against_oracle(sol, _data(sol, 5, dtype), grad_random(sol, 11, dtype), dtype, name)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed", [3, 8])
def test_random_structures_with_elimination_ranges(seed, dtype):
    sol, _, _ = solver_random(seed, fill=0.037, elim=(0, 60))
    assert len(sol.sparseEliminationRanges()) >= 2
    _check_against_oracle(sol, _data(sol, seed, dtype), grad_random(sol, seed + 1, dtype), dtype, "random%d" % seed)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["mixed_owners", "forest", "width129"])
def test_chain_with_factor_adjoint_is_the_zsz_projection(name, dtype):
    sol, _ = build_case(name)
    data = _data(sol, 6, dtype)
    grad = grad_random(sol, 12, dtype)
    L, Z = _factor_and_z(sol, data)
    g = _adjoint(sol, L, Z, to_dev(grad))
    sol.factorAdjoint(L, g)
    want = zsz_projection(sol, dense_factor(sol, data), grad)
    err = rel_error(g.cpu().numpy(), want)
    print("%s %s: chain rel. error %.3e" % (name, np.dtype(dtype).name, err))
    assert err < TOL[dtype], err


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_members_match_their_own_oracle(dtype):
    """batches of 1, 2, 5 and 17 with a gradient of their own per member.  The scatter uses atomics: no
    bitwise comparison with the single call"""
    sol, _ = build_case("mixed_owners")
    data = _data(sol, 2, dtype)
    L, Z = _factor_and_z(sol, data)
    Ld = dense_factor(sol, data)
    coords = element_coords(sol)
    grads = [grad_random(sol, 100 + q, dtype) for q in range(17)]
    wants = [dense_lbar(sol, Ld, g, coords) for g in grads]
    for B_ in (1, 2, 5, 17):
        Ls = [L.clone() for _ in range(B_)]
        Zs = [Z.clone() for _ in range(B_)]
        gs = [to_dev(grads[q]) for q in range(B_)]
        sol.selectedInverseAdjoint(Ls, Zs, gs)
        torch.cuda.synchronize()
        for q in range(B_):
            err = rel_error(gs[q].cpu().numpy(), wants[q])
            assert err < TOL[dtype], (B_, q, err)
            assert torch.equal(Ls[q], L) and torch.equal(Zs[q], Z)


def test_batch_in_chunks_with_shared_factor():
    """a batch of 5 in chunks of 2, one L and one Z read by every member (no bitwise comparison: atomics)"""
    sol, _ = build_case("width129")
    data = _data(sol, 4, np.float64)
    L, Z = _factor_and_z(sol, data)
    Ld = dense_factor(sol, data)
    coords = element_coords(sol)
    grads = [grad_random(sol, 7 + q) for q in range(5)]
    c0 = sol.runCounters()["selinv_chunks"]
    sol._testSetSelInvBatchChunk(2)
    try:
        gs = [to_dev(g) for g in grads]
        sol.selectedInverseAdjoint([L] * 5, [Z] * 5, gs)
    finally:
        sol._testSetSelInvBatchChunk(0)
    torch.cuda.synchronize()
    assert sol.runCounters()["selinv_chunks"] - c0 == 3
    for q in range(5):
        err = rel_error(gs[q].cpu().numpy(), dense_lbar(sol, Ld, grads[q], coords))
        assert err < TOL[np.float64], (q, err)


# ---- full size, without a dense oracle -----------------------------------------------------------
def _full_size(which):
    if which == "grid82":
        ss = T.gen_grid(82, 82, 1.0, 2, 37)
    else:
        ss = T.gen_meridians(4, 1500, 0.5, 120, 600, 2, 2, 37)
    sol = B.create_solver(B.Settings(), np.full(ss.order(), 3, dtype=np.int64), ss)
    data = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
    sol.damp(data, 0.0, sol.order() * 1.2)
    return sol, data


def _weights_of_a(sol, data):
    """slot weights with S = A: A_ii on the diagonal slots, A_ij on both slots of an off-diagonal element
    of a diagonal block, 2 A_ij elsewhere"""
    sk = sol.skel()
    ls = sk["lumpStart"]
    w = (ls[1:] - ls[:-1]).astype(np.int64)
    d0 = sk["chainData"][sk["chainColPtr"][:-1]].astype(np.int64)
    g = 2.0 * data
    for width in np.unique(w):
        i, j = np.tril_indices(int(width), -1)
        starts = d0[w == width][:, None]
        lo, up = (starts + (i * width + j)[None, :]).ravel(), (starts + (j * width + i)[None, :]).ravel()
        g[lo] = data[lo]
        g[up] = data[lo]
    dg = sol.diagOffsets()
    g[dg] = data[dg]
    return g


@pytest.mark.parametrize("which", ["grid82", "meri"])
def test_full_size_weights_of_a_give_minus_z(which):
    """S = A: -Z S Z = -A^-1, so the chain gives patternGrad(Z, zScale = -1)"""
    sol, data = _full_size(which)
    L, Z = _factor_and_z(sol, data)
    g = _adjoint(sol, L, Z, to_dev(_weights_of_a(sol, data)))
    sol.factorAdjoint(L, g)
    want = torch.empty_like(L)
    sol.patternGrad(want, Z=Z, zScale=-torch.ones(1, dtype=L.dtype, device="cuda"))
    err = rel_error(g.cpu().numpy(), want.cpu().numpy())
    print("%s: S = A rel. error %.3e" % (which, err))
    assert err < 1e-10, err


@pytest.mark.parametrize("which", ["grid82", "meri"])
def test_full_size_finite_difference(which):
    sol, data = _full_size(which)
    low = torch.as_tensor(sol.lowerMask(), device="cuda")
    rng = np.random.default_rng(5)
    Wt = to_dev(rng.uniform(-1, 1, sol.dataSize()))  # every slot, mirrors included
    dirn = to_dev(rng.uniform(-1, 1, sol.dataSize())) * low
    d0 = to_dev(data)

    def f(d):
        L = d.clone()
        sol.factor(L)
        Z = L.clone()
        sol.selectedInverse(Z)
        return L, Z, float(torch.dot(Wt, Z))

    L, Z, _ = f(d0)
    g = _adjoint(sol, L, Z, Wt)
    sol.factorAdjoint(L, g)
    h = 1e-4
    fd = (f(d0 + h * dirn)[2] - f(d0 - h * dirn)[2]) / (2 * h)
    an = float(torch.dot(g, dirn))
    scale = float(torch.dot(g.abs(), dirn.abs()))
    print("%s: fd %.12e analytic %.12e scale %.3e" % (which, fd, an, scale))
    assert abs(fd - an) < 1e-6 * scale, (fd, an, scale)


# ---- refusals ------------------------------------------------------------------------------------
def _rc(fn, *args):
    rc = fn(*args)
    return rc, B._lib.load().bsp_last_error().decode()


def test_selected_inverse_adjoint_refusals():
    sol, _ = build_case("mixed_owners")
    lib, h = sol._lib, sol._h
    ds = sol.dataSize()
    L = torch.ones(ds, dtype=torch.float64, device="cuda")
    Z = torch.full((ds,), 2.0, dtype=torch.float64, device="cuda")
    g = torch.zeros(3 * ds, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p
    lp, zp, gp = L.data_ptr(), Z.data_ptr(), g.data_ptr()
    launches = sol.runCounters()["selinv_launches"]
    for fn in (lib.bsp_selected_inverse_adjoint_f64, lib.bsp_selected_inverse_adjoint_f32):
        assert _rc(fn, h, p(None), p(zp), p(gp))[0] != 0
        assert _rc(fn, h, p(lp), p(None), p(gp))[0] != 0
        assert _rc(fn, h, p(lp), p(zp), p(None))[0] != 0
        rc, msg = _rc(fn, h, p(lp), p(zp), p(lp))
        assert rc != 0 and "overlaps" in msg, msg
        rc, msg = _rc(fn, h, p(lp), p(zp), p(zp))
        assert rc != 0 and "overlaps" in msg, msg
    arr = lambda *xs: (p * len(xs))(*[p(x) for x in xs])
    for fn in (lib.bsp_selected_inverse_adjoint_batched_f64, lib.bsp_selected_inverse_adjoint_batched_f32):
        rc, msg = _rc(fn, h, arr(lp), arr(zp), arr(gp), ctypes.c_int32(0))
        assert rc != 0 and "empty" in msg, msg
        assert _rc(fn, h, None, arr(zp), arr(gp), ctypes.c_int32(1))[0] != 0
        assert _rc(fn, h, arr(lp), None, arr(gp), ctypes.c_int32(1))[0] != 0
        assert _rc(fn, h, arr(lp), arr(zp), None, ctypes.c_int32(1))[0] != 0
        rc, msg = _rc(fn, h, arr(lp, lp), arr(zp, zp), arr(gp, None), ctypes.c_int32(2))
        assert rc != 0 and "NULL" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, lp), arr(zp, None), arr(gp, gp + 8 * ds), ctypes.c_int32(2))
        assert rc != 0 and "NULL" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, lp), arr(zp, zp), arr(gp, gp), ctypes.c_int32(2))
        assert rc != 0 and "overlap" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, lp), arr(zp, zp), arr(gp, gp + 8), ctypes.c_int32(2))
        assert rc != 0 and "overlap" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, gp + 8 * ds), arr(zp, zp), arr(gp, gp + 8 * ds), ctypes.c_int32(2))
        assert rc != 0 and "overlaps input" in msg, msg
        rc, msg = _rc(fn, h, arr(lp, lp), arr(zp, gp + 8 * ds), arr(gp, gp + 8 * ds), ctypes.c_int32(2))
        assert rc != 0 and "overlaps input" in msg, msg
    # the refused calls did no device work
    torch.cuda.synchronize()
    assert (g == 0).all() and (L == 1).all() and (Z == 2).all()
    assert sol.runCounters()["selinv_launches"] == launches
    inc, _, _ = solver_random(61, fill=0.03, elim=(0, 60), ranges=[0, 60], policy=B.AddFillForGivenElims)
    assert inc.canFactorUpToSpan() < inc.numSpans()
    d = torch.zeros(inc.dataSize(), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="complete factor"):
        inc.selectedInverseAdjoint(d, d.clone(), d.clone())
