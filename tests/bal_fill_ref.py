"""The ordered Hessian fill of the BAL pipeline (bsp_bal_fill_ordered_*): a numpy model of the documented
summation order, the boundary scenes of its kernels, and a block-wise long-double reference.

The model is written from the text of csrc/bal_pipeline.h / DESIGN.md section 9 ("Ordered fill"), not from
the kernels.  It reads the plan's tables (BalFillPlan._testTables) and takes every sum in the stated order in
float64 -- numpy rounds every product and every sum once and fuses nothing:

    term(o; a, b)  = fl(fl(J0a J0b) + fl(J1a J1b)),  gradient term fl(fl(J0a r0) + fl(J1a r1))
    pair block / point block / point gradient: left fold from +0.0 over the run / the point's list
    camera block / gradient: per chunk, lane l of W folds the positions l, l + W, .. from +0.0; the W lane sums
        fold by halving (h = W / 2 .. 1: T[l] += T[l + h] for l < h); the chunk partials fold left from +0.0
        in chunk order; the strict upper triangle of the block gets the sums of the lower
    applied once: data[e] = data[e] + T(S) in T arithmetic; elements nothing maps to are not touched
    damping (lam != 0): d <- fma(d, fl(1 + lam), fl(lam * T(1e-3))) in T, ONE rounding: the pass is the atomic
        fill's damping kernel, whose d (1 + lam) + 1e-3 lam the compiler contracts

Only tests/ may import this file.  Nothing here touches the GPU."""
from fractions import Fraction

import numpy as np

L = np.longdouble
C, W = 128, 4   # kBalFillChunk, kBalFillLanes of csrc/bal_fill_plan.h (the plan's info reports them)


# ---- the model ---------------------------------------------------------------------------------------
def _round_to(fr, dtype):
    """the Fraction rounded to nearest-even in dtype"""
    x = float(fr)   # correctly rounded to float64
    if np.dtype(dtype) == np.float64:
        return np.float64(x)
    c = np.float32(x)
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    dist = [abs(Fraction(float(v)) - fr) for v in cands]
    best = min(dist)
    pick = [v for v, d in zip(cands, dist) if d == best]
    if len(pick) > 1:
        pick = [v for v in pick if int(np.array([v]).view(np.uint32)[0]) % 2 == 0]
    return pick[0]


def damp(data, diag_idx, lam, dtype):
    """d <- fma(d, fl(1 + lam), fl(lam * T(1e-3))) on the listed elements, in place"""
    T = np.dtype(dtype).type
    lamT = T(lam)
    m, c = Fraction(float(T(1) + lamT)), Fraction(float(lamT * T(1e-3)))
    for i in diag_idx:
        data[i] = _round_to(Fraction(float(data[i])) * m + c, dtype)


def _terms(A0, B0, A1, B1):
    """fl(fl(A0 x B0) + fl(A1 x B1)) for every pair of columns: the outer products round each product once"""
    return np.multiply.outer(A0, B0) + np.multiply.outer(A1, B1)


def model_fill(tab, Jc, Jp, res, prior, dtype, lam, diag_idx=None, with_grad=True):
    """(data, grad) after one ordered fill of the priors (grad None when with_grad is False).  tab: the plan's
    tables; Jc (n, 2, cs), Jp (n, 2, 3), res (n, 2) float64; diag_idx: the data indices of every diagonal
    entry (for the damping pass)"""
    T = np.dtype(dtype).type
    cs = tab["camSize"]
    Jc = np.asarray(Jc, dtype=np.float64).reshape(-1, 2, cs)
    Jp = np.asarray(Jp, dtype=np.float64).reshape(-1, 2, 3)
    res = np.asarray(res, dtype=np.float64).reshape(-1, 2)
    data = np.array(prior[0], dtype=dtype, copy=True)
    grad = np.array(prior[1], dtype=dtype, copy=True) if with_grad else None
    ar3, arc = np.arange(3), np.arange(cs)
    # pairs
    for q in range(tab["nPairs"]):
        S = np.zeros((cs, 3))
        for x in range(tab["pairPtr"][q], tab["pairPtr"][q + 1]):
            o = tab["ptObs"][x]
            S = S + _terms(Jc[o, 0], Jp[o, 0], Jc[o, 1], Jp[o, 1])
        st = tab["pairStride"][q]
        idx = (ar3[None, :] * st + arc[:, None]) if tab["pairFlip"][q] else (arc[:, None] * st + ar3[None, :])
        idx = tab["pairOff"][q] + idx
        data[idx] = data[idx] + S.astype(dtype)
    # points
    for p in range(tab["numPts"]):
        x0, x1 = tab["ptPtr"][p], tab["ptPtr"][p + 1]
        if x0 == x1:
            continue
        S, G = np.zeros((3, 3)), np.zeros(3)
        for x in range(x0, x1):
            o = tab["ptObs"][x]
            S = S + _terms(Jp[o, 0], Jp[o, 0], Jp[o, 1], Jp[o, 1])
            G = G + (Jp[o, 0] * res[o, 0] + Jp[o, 1] * res[o, 1])
        idx = tab["ptDiagOff"][p] + ar3[:, None] * tab["ptDiagStride"][p] + ar3[None, :]
        data[idx] = data[idx] + S.astype(dtype)
        if with_grad:
            g = tab["ptStart"][p] + ar3
            grad[g] = grad[g] + G.astype(dtype)
    # cameras
    for c in range(tab["numCams"]):
        k0, k1 = tab["camChunkPtr"][c], tab["camChunkPtr"][c + 1]
        if k0 == k1:
            continue
        S, G = np.zeros((cs, cs)), np.zeros(cs)
        for k in range(k0, k1):
            assert tab["chunkCam"][k] == c
            pos = tab["camObs"][tab["chunkBegin"][k]:tab["chunkEnd"][k]]
            TS, TG = [], []
            for l in range(tab["W"]):
                s, g = np.zeros((cs, cs)), np.zeros(cs)
                for o in pos[l::tab["W"]]:
                    s = s + _terms(Jc[o, 0], Jc[o, 0], Jc[o, 1], Jc[o, 1])
                    g = g + (Jc[o, 0] * res[o, 0] + Jc[o, 1] * res[o, 1])
                TS.append(s)
                TG.append(g)
            h = tab["W"] // 2
            while h > 0:
                for l in range(h):
                    TS[l] = TS[l] + TS[l + h]
                    TG[l] = TG[l] + TG[l + h]
                h //= 2
            S = S + TS[0]
            G = G + TG[0]
        S = np.tril(S) + np.tril(S, -1).T   # element (b, a) gets the sum of (a, b)
        idx = tab["camDiagOff"][c] + arc[:, None] * tab["camDiagStride"][c] + arc[None, :]
        data[idx] = data[idx] + S.astype(dtype)
        if with_grad:
            g = tab["camStart"][c] + arc
            grad[g] = grad[g] + G.astype(dtype)
    if T(lam) != 0:
        damp(data, diag_idx, lam, dtype)
    return data, grad


# ---- boundary scenes ---------------------------------------------------------------------------------
EDGE_COUNTS = (W - 1, W, W + 1, C - 1, C, C + 1, 2 * C + 3)
_CASES = {}


def edge_case(cam_size):
    """camera k sees the points 0 .. EDGE_COUNTS[k] - 1 (so a point is seen by 1 to 7 cameras); one more camera
    and one more point that nobody observes.  Dict like bal_ref.fill_case, without the dense normal equations."""
    if cam_size not in _CASES:
        import baspacho_amd as B
        import bal_ref as R
        from baspacho_amd import bal
        from oracle import bal_model
        nc, npt = len(EDGE_COUNTS) + 1, max(EDGE_COUNTS) + 1
        oc = np.concatenate([np.full(n, k) for k, n in enumerate(EDGE_COUNTS)]).astype(np.int64)
        op = np.concatenate([np.arange(n) for n in EDGE_COUNTS]).astype(np.int64)
        prob = bal.synth_scene_for(nc, npt, oc, op, seed=11)
        sizes, ss, ranges = bal.bal_structure(prob, cam_size=cam_size)
        sol = B.create_solver(B.Settings(), sizes, ss, ranges)
        lin = bal_model.linearize if cam_size == 9 else bal_model.linearize_se3
        res, Jc, Jp = lin(prob.cams[prob.obs_cam], prob.pts[prob.obs_pt], prob.obs_xy)
        _CASES[cam_size] = {"prob": prob, "sol": sol, "res": res, "Jc": Jc, "Jp": Jp, "cam_size": cam_size,
                            "lay": R.layout(sol, npt, nc, cam_size)}
    return _CASES[cam_size]


def with_bad_observations(c):
    """the list of test_out_of_range_observations_are_skipped (tests/test_bal_edges_gpu.py): nine observations
    with an index out of range mixed into the 30x8 scene, with random Jacobians and residuals of their own"""
    prob = c["prob"]
    nc, npt, n = prob.num_cams, prob.num_pts, len(prob.obs_cam)
    bad = [(-1, 0), (0, -1), (nc, 0), (0, npt), (0, nc), (2 ** 40, 0), (0, 2 ** 40), (-1, -1), (nc, npt)]
    at = [0, 1, 5, 42, 43, 44, 67, n - 1, n]
    rng = np.random.default_rng(9)
    oc, op = np.insert(prob.obs_cam, at, [b[0] for b in bad]), np.insert(prob.obs_pt, at, [b[1] for b in bad])
    Jc = np.insert(c["Jc"], at, rng.uniform(-50, 50, (len(bad),) + c["Jc"].shape[1:]), axis=0)
    Jp = np.insert(c["Jp"], at, rng.uniform(-50, 50, (len(bad), 2, 3)), axis=0)
    res = np.insert(c["res"], at, rng.uniform(-5, 5, (len(bad), 2)), axis=0)
    skipped = (oc < 0) | (oc >= nc) | (op < 0) | (op >= npt)
    assert int(skipped.sum()) == len(bad) and np.array_equal(oc[~skipped], prob.obs_cam)
    return oc, op, Jc, Jp, res, skipped


# ---- block-wise reference ------------------------------------------------------------------------------
def blockwise_expected(num_pts, num_cams, cam_size, obs_cam, obs_pt, Jc, Jp, res, lay, dtype):
    """bal_ref.expected_fill's dict (H, Hbound, Htouched, HA, g, gbound, gtouched, gA in the solver's layout)
    from block-wise np.longdouble sums, without the dense J: every term of every observation is added at the
    data element that lay (the skeleton's own coordinates) places at its dense position.  Same bound:
    2 (n + 1) eps_T sum |J_a| |J_b| with n the number of observations that reach the element."""
    cs, n = cam_size, 3 * num_pts + cam_size * num_cams
    Jc = np.asarray(Jc, dtype=L).reshape(-1, 2, cs)
    Jp = np.asarray(Jp, dtype=L).reshape(-1, 2, 3)
    r = np.asarray(res, dtype=L).reshape(-1, 2)
    oc, op = np.asarray(obs_cam, dtype=np.int64), np.asarray(obs_pt, dtype=np.int64)
    size = len(lay["rows"])
    stored = np.nonzero(lay["lower"])[0]
    keys = lay["rows"][stored] * n + lay["cols"][stored]
    order = np.argsort(keys)
    keys, stored = keys[order], stored[order]
    assert len(np.unique(keys)) == len(keys)

    def find(rows, cols):
        k = rows * n + cols
        at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        return np.where(keys[at] == k, stored[at], -1)

    H, A, N = np.zeros(size, dtype=L), np.zeros(size, dtype=L), np.zeros(size, dtype=np.int64)
    cam0 = (3 * num_pts + cs * oc)[:, None, None] + np.arange(cs)[None, :, None]   # (nobs, cs, 1)
    pt0 = (3 * op)[:, None, None] + np.arange(3)[None, :, None]                     # (nobs, 3, 1)

    def add(rows, cols, X, Y, both_ways):
        v = X[:, 0, :, None] * Y[:, 0, None, :] + X[:, 1, :, None] * Y[:, 1, None, :]
        a = np.abs(X[:, 0, :, None] * Y[:, 0, None, :]) + np.abs(X[:, 1, :, None] * Y[:, 1, None, :])
        rows, cols = np.broadcast_arrays(rows, cols)
        at = find(rows, cols)
        if both_ways:
            at = np.where(at >= 0, at, find(cols, rows))
        assert (at >= 0).all(), "an observation's element is not stored"
        np.add.at(H, at.ravel(), v.ravel())
        np.add.at(A, at.ravel(), a.ravel())
        np.add.at(N, at.ravel(), 1)

    add(cam0, cam0.transpose(0, 2, 1), Jc, Jc, False)
    add(pt0, pt0.transpose(0, 2, 1), Jp, Jp, False)
    add(cam0, pt0.transpose(0, 2, 1), Jc, Jp, True)
    eps = L(np.finfo(dtype).eps)
    touched = N > 0
    g, gA, gN = np.zeros(n, dtype=L), np.zeros(n, dtype=L), np.zeros(n, dtype=np.int64)
    for idx, X in ((cam0[:, :, 0], Jc), (pt0[:, :, 0], Jp)):
        np.add.at(g, idx.ravel(), (X[:, 0] * r[:, 0:1] + X[:, 1] * r[:, 1:2]).ravel())
        np.add.at(gA, idx.ravel(), (np.abs(X[:, 0] * r[:, 0:1]) + np.abs(X[:, 1] * r[:, 1:2])).ravel())
        np.add.at(gN, idx.ravel(), 1)
    out = {"H": H, "Hbound": 2 * (N + 1) * eps * A * touched, "Htouched": touched, "HA": A}
    for name, v in (("g", g), ("gbound", 2 * (gN + 1) * eps * gA), ("gtouched", gN > 0), ("gA", gA)):
        o = np.zeros(n, dtype=v.dtype)
        o[lay["vec"]] = v
        out[name] = o
    return out


def check_fill(diag, dtype, exp, prior, got, gotg, lam, what):
    """every element of data and grad against bal_ref.expected_fill's dict: touched ones within the bound of
    prior + H (diagonal entries damped by lam: within 4 eps_T of |h| (1 + lam) + 1e-3 lam on top of the carried
    bound), all others bitwise the prior.  The yardstick of the atomic fill's test, restated."""
    from known_factor import bitwise_equal
    eps = L(np.finfo(dtype).eps)
    want = prior[0].astype(L) + exp["H"]
    bound = np.array(exp["Hbound"], dtype=L, copy=True)
    same = ~exp["Htouched"]
    if lam != 0:
        bound[diag] = bound[diag] * (1 + L(lam)) + 4 * eps * (np.abs(want[diag]) * (1 + L(lam)) + L(1e-3) * L(lam))
        want[diag] = want[diag] * (1 + L(lam)) + L(1e-3) * L(lam)
        same[diag] = False
    assert bitwise_equal(got[same], prior[0][same]), (what, "an element no observation maps to changed")
    err = np.abs(got.astype(L) - want)
    assert np.isfinite(got).all() and np.all(err <= bound), (what, int((err > bound).sum()), "data elements miss",
                                                              float((err / np.maximum(bound, 1e-300)).max()))
    if gotg is None:
        return
    wantg = prior[1].astype(L) + exp["g"]
    assert bitwise_equal(gotg[~exp["gtouched"]], prior[1][~exp["gtouched"]]), (what, "an untouched grad entry changed")
    errg = np.abs(gotg.astype(L) - wantg)
    assert np.isfinite(gotg).all() and np.all(errg <= exp["gbound"]), (what, int((errg > exp["gbound"]).sum()),
                                                                     "grad entries miss")
