"""The BAL pipeline kernels (csrc/bal_pipeline.hip through baspacho_amd/bal.py) against the independent
reference of tests/bal_ref.py, on framed buffers.

Linearisation: every case of bal_ref.LIN_CASES in both parameterisations, against 70-digit central
differences.  Bound bal_ref.LIN_BOUND = 8.3e-14 = 8 x the worst error of the float64 host model against the
same reference (1.03e-14 Jacobian, 3.1e-16 residual; tests/test_bal_ref_cpu.py), on errors scaled per
observation and column (Jacobians) and by |projection| + |xy| (residuals).

Hessian fill: expected values from dense J^T J in np.longdouble, mapped to the layout by the skeleton and
scalarPermutation().  Every touched element: |got - prior - H| <= 2 (n + 1) eps_T sum |J_a| |J_b| (derived
in bal_ref.expected_fill); every other element bitwise the prior."""
import numpy as np
import pytest
import torch

import bal_ref as R
from baspacho_amd import bal
from buffer_edges import Frame, framed, is_sentinel, bitwise_equal

pytestmark = pytest.mark.gpu
L = np.longdouble


def _i64(a):
    """int64 indices as the float64 words a Frame holds"""
    return np.ascontiguousarray(a, dtype=np.int64).view(np.float64)


def _as_i64(t):
    return t.view(torch.int64)


# ---- 4a: linearisation ---------------------------------------------------------------------------------
LIN_RUNS = [("generic", n) for n in R.OBS_COUNTS] + [(name, None) for name in R.LIN_CASES if name != "generic"]
_LIN_SOLVERS = {}


def _lin_solver(name, cam_size):
    import baspacho_amd as B
    if (name, cam_size) not in _LIN_SOLVERS:
        sizes, ss, ranges = bal.bal_structure(R.lin_problem(name), cam_size=cam_size)
        _LIN_SOLVERS[name, cam_size] = B.create_solver(B.Settings(), sizes, ss, ranges)
    return _LIN_SOLVERS[name, cam_size]


@pytest.mark.parametrize("name,count", LIN_RUNS, ids=["%s-%s" % r for r in LIN_RUNS])
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_linearisation_against_the_reference(param, name, count):
    prob = R.lin_problem(name)
    n = len(prob.obs_cam) if count is None else count
    cs = 9 if param == "bal9" else 6
    ref = tuple(a[:n] for a in R.lin_reference(name, param))
    fin = framed(np.float64, [_i64(prob.obs_cam[:n]), _i64(prob.obs_pt[:n]), prob.obs_xy[:n], prob.cams, prob.pts])
    fout = Frame([2 * n, 2 * cs * n, 6 * n], np.float64)
    pipe = bal.DevicePipeline(prob, _lin_solver(name, cs), param=param)
    pipe.obs_cam, pipe.obs_pt, pipe.obs_xy = _as_i64(fin.view(0)), _as_i64(fin.view(1)), fin.view(2)
    pipe.cams, pipe.pts = fin.view(3), fin.view(4)
    pipe.res, pipe.Jc, pipe.Jp, pipe.n_obs = fout.view(0), fout.view(1), fout.view(2), n
    pipe.linearize()
    torch.cuda.synchronize()
    fout.assert_intact(what="linearize outputs")
    fin.assert_intact(read_only=range(5), what="linearize inputs")
    got = [fout.host(k) for k in range(3)]
    for k, a in enumerate(got):
        assert not is_sentinel(a).any(), ("an output word was not written", k, int(is_sentinel(a).sum()))
    eres, ejac = R.lin_errors(got, ref)
    print("%s %s n=%d: residual %.2e Jacobian %.2e (bound %.1e)" % (param, name, n, eres, ejac, R.LIN_BOUND))
    assert eres <= R.LIN_BOUND and ejac <= R.LIN_BOUND, (eres, ejac)
    if name == "special" and param == "se3":
        res, Jc, Jp = got[0].reshape(n, 2), got[1].reshape(n, 12), got[2].reshape(n, 6)
        for o, z in R.SPECIAL_Z.items():
            if z > 0.01:   # in front of the image plane: the fixed residual, bit for bit, and zero Jacobians
                assert bitwise_equal(res[o], np.array([25.0, 0.0]))
                assert bitwise_equal(Jc[o], np.zeros(12)) and bitwise_equal(Jp[o], np.zeros(6))
            else:
                assert np.isfinite(res[o]).all() and tuple(res[o]) != (25.0, 0.0) and Jc[o].all() and Jp[o].any()


# ---- 4b: Hessian fill ----------------------------------------------------------------------------------
def _run_fill(c, dtype, lam, prior, obs=None, n_obs=None, want_dbg=False):
    """one fill_hessian call on framed buffers; obs = (obs_cam, obs_pt, Jc, Jp, res) replaces the scene's
    own list.  Checks the frames and returns (data, grad, dbg rows as int64 or None)."""
    prob, sol = c["prob"], c["sol"]
    oc, op, Jc, Jp, res = obs if obs is not None else (prob.obs_cam, prob.obs_pt, c["Jc"], c["Jp"], c["res"])
    n = len(oc) if n_obs is None else n_obs
    fin = framed(np.float64, [_i64(oc), _i64(op), Jc, Jp, res])
    fdat = framed(dtype, prior)
    fdbg = Frame([7 * len(oc)], np.float64) if want_dbg else None
    pipe = bal.DevicePipeline(prob, sol, param="bal9" if c["cam_size"] == 9 else "se3")
    pipe.obs_cam, pipe.obs_pt = _as_i64(fin.view(0)), _as_i64(fin.view(1))
    pipe.Jc, pipe.Jp, pipe.res, pipe.n_obs = fin.view(2), fin.view(3), fin.view(4), n
    pipe.fill_hessian(fdat.view(0), fdat.view(1), lam, _as_i64(fdbg.view(0)) if want_dbg else None)
    torch.cuda.synchronize()
    fin.assert_intact(read_only=range(5), what="fill inputs")
    fdat.assert_intact(what="data and grad")
    dbg = None
    if want_dbg:
        fdbg.assert_intact(what="dbg")
        dbg = fdbg.host(0).view(np.int64).reshape(-1, 7)
    return fdat.host(0), fdat.host(1), dbg


def _check_fill(c, dtype, exp, prior, got, gotg, lam, what):
    """every element of data and grad: touched ones within the bound of prior + H (diagonal entries damped
    by lam: h (1 + lam) + 1e-3 lam within 4 eps_T of |h| (1 + lam) + 1e-3 lam, the two terms may cancel, on
    top of the carried bound), all others bitwise the prior"""
    eps = L(np.finfo(dtype).eps)
    diag = c["lay"]["diag"]
    want = prior[0].astype(L) + exp["H"]
    bound = exp["Hbound"].copy()
    same = ~exp["Htouched"]
    if lam != 0:
        bound[diag] = bound[diag] * (1 + L(lam)) + 4 * eps * (np.abs(want[diag]) * (1 + L(lam)) + L(1e-3) * L(lam))
        want[diag] = want[diag] * (1 + L(lam)) + L(1e-3) * L(lam)
        same[diag] = False
    assert bitwise_equal(got[same], prior[0][same]), (what, "an element no observation maps to changed")
    err = np.abs(got.astype(L) - want)
    assert np.isfinite(got).all() and np.all(err <= bound), (what, int((err > bound).sum()), "data elements miss",
                                                              float((err / np.maximum(bound, 1e-300)).max()))
    wantg = prior[1].astype(L) + exp["g"]
    assert bitwise_equal(gotg[~exp["gtouched"]], prior[1][~exp["gtouched"]]), (what, "an untouched grad entry changed")
    errg = np.abs(gotg.astype(L) - wantg)
    assert np.isfinite(gotg).all() and np.all(errg <= exp["gbound"]), (what, int((errg > exp["gbound"]).sum()),
                                                                     "grad entries miss")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cam_size", [9, 6])
@pytest.mark.parametrize("name", R.FILL_SCENES)
def test_fill_against_dense_normal_equations(name, cam_size, dtype):
    c = R.fill_case(name, cam_size)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=len(name) + cam_size)
    assert exp["Htouched"].any()
    for lam in (0.0, 0.3):
        got, gotg, dbg = _run_fill(c, dtype, lam, prior, want_dbg=cam_size == 9)
        _check_fill(c, dtype, exp, prior, got, gotg, lam, (name, cam_size, lam))
        if dbg is not None and name in R.FLIPPED:   # the transposed store runs (and, where listed, the plain one)
            assert (len(dbg), int(dbg[:, 2].sum())) == R.FLIPPED[name]
            assert set(dbg[:, 2].tolist()) <= {0, 1}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cam_size", [9, 6])
def test_no_observations_damps_the_prior_only_or_writes_nothing(cam_size, dtype):
    """numObs = 0: with lambda = 0 nothing is launched and nothing written (negative zeros on the diagonal
    survive, which a damping pass would turn positive); with lambda = 0.3 every diagonal entry becomes
    h (1 + lambda) + 1e-3 lambda within 4 eps_T and no other word changes.  The same on the output of a
    fill: lambda = 0 leaves it bitwise as it is."""
    c = R.fill_case("30x8", cam_size)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=5)
    diag = c["lay"]["diag"]
    prior[0][diag[::5]] = -0.0
    nothing = {k: np.zeros_like(v) for k, v in exp.items()}
    nothing["Htouched"], nothing["gtouched"] = np.zeros_like(exp["Htouched"]), np.zeros_like(exp["gtouched"])
    got, gotg, _ = _run_fill(c, dtype, 0.0, prior, n_obs=0)
    assert bitwise_equal(got, prior[0]) and bitwise_equal(gotg, prior[1])
    got, gotg, _ = _run_fill(c, dtype, 0.3, prior, n_obs=0)
    _check_fill(c, dtype, nothing, prior, got, gotg, 0.3, "numObs = 0, lambda = 0.3")
    eps = np.finfo(dtype).eps
    h = prior[0][diag].astype(L)
    assert np.all(np.abs(got[diag].astype(L) - (h * (1 + L(0.3)) + L(3e-4))) <= 4 * eps * (np.abs(h) * 1.3 + 3e-4))
    filled, filledg, _ = _run_fill(c, dtype, 0.0, prior)
    again, againg, _ = _run_fill(c, dtype, 0.0, [filled, filledg], n_obs=0)
    assert bitwise_equal(again, filled) and bitwise_equal(againg, filledg)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("cam_size", [9, 6])
def test_out_of_range_observations_are_skipped(cam_size, dtype):
    """observations with a camera or point index of -1, numPts (as point), numCams (as camera or point) or
    2^40 mixed into the list: the result is that of the list without them, to the same bound; their dbg rows
    are never written"""
    c = R.fill_case("30x8", cam_size)
    prob = c["prob"]
    nc, npt, n = prob.num_cams, prob.num_pts, len(prob.obs_cam)
    assert nc > npt
    bad = [(-1, 0), (0, -1), (nc, 0), (0, npt), (0, nc), (2 ** 40, 0), (0, 2 ** 40), (-1, -1), (nc, npt)]
    at = [0, 1, 5, 42, 43, 44, 67, n - 1, n]   # where they go in: first, inside and across launch blocks of 4, last
    rng = np.random.default_rng(9)
    oc, op = np.insert(prob.obs_cam, at, [b[0] for b in bad]), np.insert(prob.obs_pt, at, [b[1] for b in bad])
    Jc = np.insert(c["Jc"], at, rng.uniform(-50, 50, (len(bad),) + c["Jc"].shape[1:]), axis=0)
    Jp = np.insert(c["Jp"], at, rng.uniform(-50, 50, (len(bad), 2, 3)), axis=0)
    res = np.insert(c["res"], at, rng.uniform(-5, 5, (len(bad), 2)), axis=0)
    skipped = (oc < 0) | (oc >= nc) | (op < 0) | (op >= npt)
    assert int(skipped.sum()) == len(bad) and np.array_equal(oc[~skipped], prob.obs_cam)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=13)
    for lam in (0.0, 0.3):
        got, gotg, dbg = _run_fill(c, dtype, lam, prior, obs=(oc, op, Jc, Jp, res), want_dbg=cam_size == 9)
        _check_fill(c, dtype, exp, prior, got, gotg, lam, ("out of range", cam_size, lam))
        if dbg is not None:
            words = dbg.view(np.float64)
            assert is_sentinel(words[skipped]).all() and not is_sentinel(words[~skipped]).any()


def test_device_accessor_answers_are_the_host_accessors_on_a_flipped_scene():
    """dbg of the 40 x 6 scene (204 of 240 blocks flipped) against Solver.blockOffset / diagBlockOffset"""
    c = R.fill_case("40x6", 9)
    prob, sol = c["prob"], c["sol"]
    exp = R.expected_fill(c["ne"], c["lay"], np.float64)
    _, _, dbg = _run_fill(c, np.float64, 0.0, R.prior_for(exp, np.float64, seed=1), want_dbg=True)
    want = np.array([sol.blockOffset(prob.num_pts + int(cam), int(pt))[:2] +
                     (int(sol.blockOffset(prob.num_pts + int(cam), int(pt))[2]),) +
                     sol.diagBlockOffset(prob.num_pts + int(cam)) + sol.diagBlockOffset(int(pt))
                     for cam, pt in zip(prob.obs_cam, prob.obs_pt)], dtype=np.int64)
    assert np.array_equal(dbg, want)
    assert set(dbg[:, 2].tolist()) == {0, 1}


# ---- 4c: stream ----------------------------------------------------------------------------------------
def test_pipeline_runs_on_the_solvers_stream():
    """setStream(s) for a torch side stream: with tens of ms of matmuls queued on s, then the copies that
    bring the true cameras and points into buffers that held NaN, linearize() and fill_hessian() must run
    after them on s (no host synchronisation in between).  On the null stream they would read the NaN."""
    c = R.fill_case("16x400", 9)
    prob, sol = c["prob"], c["sol"]
    lam = 0.3
    dev = "cuda"

    def buffers():
        return (torch.zeros(sol.dataSize(), dtype=torch.float64, device=dev),
                torch.zeros(sol.order(), dtype=torch.float64, device=dev))
    pipe0 = bal.DevicePipeline(prob, sol)
    H0, g0 = buffers()
    pipe0.linearize()
    pipe0.fill_hessian(H0, g0, lam)
    pipe = bal.DevicePipeline(prob, sol)
    true_cams, true_pts = pipe.cams.clone(), pipe.pts.clone()
    pipe.cams.fill_(float("nan"))
    pipe.pts.fill_(float("nan"))
    H, g = buffers()
    A = torch.randn(8192, 8192, dtype=torch.float64, device=dev)
    C = torch.empty_like(A)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    sol.setStream(s)
    try:
        with torch.cuda.stream(s):
            for _ in range(4):
                torch.matmul(A, A, out=C)
            pipe.cams.copy_(true_cams)
            pipe.pts.copy_(true_pts)
            pipe.linearize()
            pipe.fill_hessian(H, g, lam)
        s.synchronize()
    finally:
        sol.setStream(None)
    torch.cuda.synchronize()
    for a, b in ((pipe.res, pipe0.res), (pipe.Jc, pipe0.Jc), (pipe.Jp, pipe0.Jp)):
        assert not torch.isnan(a).any(), "the linearisation read the buffers before the copies on the stream"
        assert torch.equal(a, b)
    exp = R.expected_fill(c["ne"], c["lay"], np.float64)
    got, want = H.cpu().numpy(), H0.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(g.cpu().numpy()).all()
    bound = exp["Hbound"].copy()
    diag = c["lay"]["diag"]
    bound[diag] = bound[diag] * (1 + L(lam)) + 4 * np.finfo(np.float64).eps * (np.abs(want[diag]) + 1e-3 * lam)
    assert np.all(np.abs(got.astype(L) - want) <= bound)
    assert np.all(np.abs(g.cpu().numpy().astype(L) - g0.cpu().numpy()) <= exp["gbound"])
    # an explicit stream= overrides the solver's
    H2, g2 = buffers()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        pipe.fill_hessian(H2, g2, lam, stream=s)
    s.synchronize()
    assert np.all(np.abs(H2.cpu().numpy().astype(L) - want) <= bound)
    del A, C
    torch.cuda.empty_cache()
