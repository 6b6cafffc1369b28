"""GPU: selected inversion at the split points of its plan, entry by entry.  Every explicit skeleton of
selinv_cases.py first asserts (on Solver._testSelInvPlan()) that it takes the path it was built for:
small item or nodes, ragged rightmost node, node boundary inside a span, split-K (nk > 1, partial last
chunk) or not.  Then every stored entry of Z is compared with inv(A) in correlation units
(selinv_ref.py).  Also: selected inversion after each way of producing a factor, and marginals() /
blockOffset() blocks of a bundle-adjustment problem against inv(H) assembled in user order."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import bal
from helpers import solver_random, spd_data, to_dev
from oracle import bal_model
from selinv_cases import build_case, case_names
from selinv_ref import corr_error, dense_reference, lump_path

pytestmark = pytest.mark.gpu

# 10x the worst value of the first MI355X runs (fp64 2.6e-15, fp32 1.2e-6, worst entry over
# test_selinv_gpu.py and test_selinv_edges_gpu.py); REF_RES bounds max|A X - I| of the reference
TOL = {np.float64: 2.5e-14, np.float32: 1e-5}
REF_RES = 1e-14


def _run(sol, data):
    import torch
    d = to_dev(data)
    sol.factor(d)
    sol.selectedInverse(d)
    torch.cuda.synchronize()
    return d.cpu().numpy().astype(np.float64)


def _check(sol, data, got, dtype, tag):
    _, want, res = dense_reference(sol, data)
    assert res < REF_RES, res
    err = corr_error(sol, got, want)
    print("selinv-err %s %s %s" % (tag, np.dtype(dtype).name, err))
    assert err.value < TOL[dtype], (tag, err)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", case_names())
def test_explicit_skeletons(name, dtype):
    sol, expect = build_case(name)
    expect(sol._testSelInvPlan())
    data = spd_data(sol, 17, dtype=dtype)
    _check(sol, data, _run(sol, data), dtype, name)


def test_factor_entry_points():
    """selected inversion after: one element of a batched factor, factorUpTo + factorFrom, the per-op
    factor, a solver rebuilt from its serialized plan, fp32 then fp64 on one solver (scratch reused),
    and a refactor: the second selected inversion of a solver is bitwise equal to a fresh solver's"""
    import torch
    sol, _, _ = solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50])
    plan = sol._testSelInvPlan()
    assert len(plan["small"]["lump"]) and len(plan["node"]["lump"])
    data = spd_data(sol, 23)
    _, want, _ = dense_reference(sol, data)

    def check(d, tag, dtype=np.float64):
        torch.cuda.synchronize()
        err = corr_error(sol, d.cpu().numpy().astype(np.float64), want)
        assert err.value < TOL[dtype], (tag, err)

    # batched factor
    ds = [to_dev(data), to_dev(spd_data(sol, 24))]
    sol.factor(ds)
    sol.selectedInverse(ds[0])
    check(ds[0], "batch")
    # factorUpTo + factorFrom
    # factorUpTo stops at a lump boundary past the sparse-elimination ranges
    mid_lump = max(int(sol.sparseEliminationRanges()[-1]), sol.numLumps() // 2)
    assert mid_lump < sol.numLumps()
    mid = int(sol.skel()["lumpToSpan"][mid_lump])
    d = to_dev(data)
    sol.factorUpTo(d, mid)
    sol.factorFrom(d, mid)
    sol.selectedInverse(d)
    check(d, "upTo+from")
    # per-op factor
    d = to_dev(data)
    sol.factorPerOp(d)
    L = d.clone()
    sol.selectedInverse(d)
    check(d, "per-op")
    # from_plan
    other = B.Solver.from_plan(sol.serialize_plan())
    d = L.clone()
    other.selectedInverse(d)
    check(d, "from_plan")
    # fp32 then fp64 on one solver
    fresh, _, _ = solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50])
    d32 = spd_data(fresh, 23, dtype=np.float32)
    _, want32, _ = dense_reference(fresh, d32)
    got32 = _run(fresh, d32)
    assert corr_error(fresh, got32, want32).value < TOL[np.float32]
    d = L.clone()
    fresh.selectedInverse(d)
    check(d, "fp64 after fp32")
    # refactor + second selected inversion == a fresh solver's, bitwise (same factor input)
    x = to_dev(spd_data(sol, 31))
    sol.factor(x)
    sol.selectedInverse(x)
    a = L.clone()
    sol.selectedInverse(a)
    newsol, _, _ = solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50])
    b = L.clone()
    newsol.selectedInverse(b)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a, d)


def _bal_problem():
    """24 cameras, 160 points: points 0..19 seen by 20 cameras each (node path for their 3-wide
    lumps), the others by 2..6 neighbouring cameras (small path)"""
    rng = np.random.default_rng(11)
    nc, npt = 24, 160
    oc, op = [], []
    for p in range(npt):
        if p < 20:
            sel = np.sort(rng.choice(nc, 20, replace=False))
        else:
            c0 = int(rng.integers(0, nc - 6))
            sel = np.unique(c0 + rng.integers(0, 6, size=int(rng.integers(2, 7))))
            if len(sel) < 2:
                sel = np.array([c0, c0 + 1])
        oc += sel.tolist()
        op += [p] * len(sel)
    return bal.synth_scene_for(nc, npt, np.array(oc), np.array(op), seed=5)


def _user_hessian(prob, Jc, Jp, lam):
    """H = J^T J with the damping of fill_hessian_host, in USER parameter order (points, then
    cameras), assembled with numpy only"""
    npt, nc = prob.num_pts, prob.num_cams
    n = 3 * npt + 9 * nc
    H = np.zeros((n, n))
    for o, (c, p) in enumerate(zip(prob.obs_cam, prob.obs_pt)):
        pi = slice(3 * p, 3 * p + 3)
        ci = slice(3 * npt + 9 * c, 3 * npt + 9 * c + 9)
        H[pi, pi] += Jp[o].T @ Jp[o]
        H[ci, ci] += Jc[o].T @ Jc[o]
        H[ci, pi] += Jc[o].T @ Jp[o]
        H[pi, ci] += Jp[o].T @ Jc[o]
    dg = np.arange(n)
    H[dg, dg] = H[dg, dg] * (1.0 + lam) + lam * 1e-3
    return H


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_user_order_marginals_and_blocks(dtype):
    import torch
    prob = _bal_problem()
    sizes, ss, elim = bal.bal_structure(prob)
    sol = B.create_solver(B.Settings(), sizes, ss, elim)
    plan = sol._testSelInvPlan()
    p2s = sol.paramToSpan()
    s2l = sol.skel()["spanToLump"]
    assert all(lump_path(plan, int(s2l[p2s[p]]))[0] == "node" for p in range(20))
    assert lump_path(plan, int(s2l[p2s[40]]))[0] == "small"
    res, Jc, Jp = bal_model.linearize(prob.cams[prob.obs_cam], prob.pts[prob.obs_pt], prob.obs_xy)
    lam = 5e-3 if dtype == np.float64 else 1.0
    data, _, _ = bal_model.fill_hessian_host(sol, prob, Jc, Jp, res, lam)
    data = data.astype(dtype)
    H = _user_hessian(prob, Jc, Jp, lam)
    if dtype == np.float32:
        H = H.astype(np.float32).astype(np.float64)
    cond = np.linalg.cond(H)
    Zu = np.linalg.inv(H)
    d = to_dev(data)
    sol.factor(d)
    sol.selectedInverse(d)
    torch.cuda.synchronize()
    Z = d.cpu().numpy().astype(np.float64)
    npt = prob.num_pts
    off = np.concatenate([[0], np.cumsum(sizes)])
    dz = np.diag(Zu)
    worst = (0.0, None)

    def upd(blk, p, q):
        nonlocal worst
        want = Zu[off[q]:off[q + 1], off[p]:off[p + 1]]
        sc = np.sqrt(np.outer(dz[off[q]:off[q + 1]], dz[off[p]:off[p + 1]]))
        e = float((np.abs(blk - want) / sc).max())
        if not e <= worst[0]:
            worst = (e, (q, p))

    params = list(range(len(sizes)))
    m = sol.marginals(d, params)
    for p in params:
        upd(m[p].cpu().numpy().astype(np.float64), p, p)
    for c, pt in set(zip(prob.obs_cam.tolist(), prob.obs_pt.tolist())):
        q, p = npt + c, pt
        o, st, fl = sol.blockOffset(q, p)
        nq, np_ = int(sizes[q]), int(sizes[p])
        if fl:
            blk = np.array([[Z[o + i * st + j] for j in range(nq)] for i in range(np_)]).T
        else:
            blk = np.array([[Z[o + i * st + j] for j in range(np_)] for i in range(nq)])
        upd(blk, p, q)
    eps = float(np.finfo(dtype).eps)
    print("selinv-err bal-user-order %s cond %.2e worst %.3e at %s" % (np.dtype(dtype).name, cond, *worst))
    if dtype == np.float64:
        assert 1e7 < cond < 1e9, cond
        assert worst[0] < 1.0 * cond * eps, (worst, cond)   # first MI355X run: 0.12 cond eps
    else:
        assert worst[0] < TOL[np.float32], (worst, cond)
