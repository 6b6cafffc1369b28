"""The ordered Hessian fill (bsp_bal_fill_ordered_* through DevicePipeline.fill_hessian_ordered) on framed
buffers: against the long-double references at the bound of the atomic fill's test (2 (n + 1) eps sum |J_a| |J_b|,
tests/bal_ref.py expected_fill), and BITWISE against the numpy model of the documented summation order
(tests/bal_fill_ref.py), on every fill scene and on the boundary scenes of its kernels."""
import numpy as np
import pytest
import torch

import bal_fill_ref as F
import bal_ref as R
from baspacho_amd import bal
from buffer_edges import framed, bitwise_equal

pytestmark = pytest.mark.gpu
L = np.longdouble
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


def _pipeline(c, obs=None):
    """a DevicePipeline of the scene; obs = (obs_cam, obs_pt) replaces the scene's own list"""
    prob = c["prob"]
    if obs is not None:
        prob = bal.BalProblem(prob.cams, prob.pts, np.asarray(obs[0], dtype=np.int64),
                              np.asarray(obs[1], dtype=np.int64), np.zeros((len(obs[0]), 2)))
    return bal.DevicePipeline(prob, c["sol"], param="bal9" if c["cam_size"] == 9 else "se3")


def _run(pipe, inputs, dtype, lam, prior, with_grad=True, twice=True):
    """fill_hessian_ordered on framed buffers (every payload at an odd element offset); checks the frames, the
    read-only inputs and, with `twice`, that a second call on the same inputs gives the same bits.  Returns
    (data, grad or None)."""
    Jc, Jp, res = inputs
    out = []
    for _ in range(2 if twice else 1):
        fin = framed(np.float64, [Jc, Jp, res])
        fdat = framed(dtype, prior if with_grad else prior[:1])
        pipe.Jc, pipe.Jp, pipe.res = fin.view(0), fin.view(1), fin.view(2)
        pipe.fill_hessian_ordered(fdat.view(0), fdat.view(1) if with_grad else None, lam)
        torch.cuda.synchronize()
        fin.assert_intact(read_only=range(3), what="ordered fill inputs")
        fdat.assert_intact(what="data and grad")
        out.append((fdat.host(0), fdat.host(1) if with_grad else None))
    if twice:
        assert bitwise_equal(out[0][0], out[1][0]), "a second call gave other bits in data"
        assert not with_grad or bitwise_equal(out[0][1], out[1][1]), "a second call gave other bits in grad"
    return out[0]


def _bitwise_the_model(pipe, c, inputs, dtype, lam, prior, got, gotg, what):
    tab = pipe.fill_plan()._testTables()
    want, wantg = F.model_fill(tab, *inputs, prior, dtype, lam, c["lay"]["diag"], with_grad=gotg is not None)
    assert bitwise_equal(got, want), (what, "data differs from the model in %d words" % int(
        (got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1).sum()))
    if gotg is not None:
        assert bitwise_equal(gotg, wantg), (what, "grad differs from the model")


@DTYPES
@pytest.mark.parametrize("cam_size", [9, 6])
@pytest.mark.parametrize("name", R.FILL_SCENES)
def test_ordered_fill_against_the_reference_and_bitwise_the_model(name, cam_size, dtype):
    c = R.fill_case(name, cam_size)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=len(name) + cam_size)
    assert exp["Htouched"].any()
    pipe = _pipeline(c)
    inputs = (c["Jc"], c["Jp"], c["res"])
    for lam in (0.0, 0.3):
        got, gotg = _run(pipe, inputs, dtype, lam, prior)
        F.check_fill(c["lay"]["diag"], dtype, exp, prior, got, gotg, lam, (name, cam_size, lam))
        _bitwise_the_model(pipe, c, inputs, dtype, lam, prior, got, gotg, (name, cam_size, lam))


@DTYPES
@pytest.mark.parametrize("cam_size", [9, 6])
def test_boundary_scene_of_the_chunks_and_lanes(cam_size, dtype):
    """cameras that see W - 1, W, W + 1, C - 1, C, C + 1 and 2 C + 3 points, a camera and a point nobody observes
    (their blocks move by damping only), with and without grad"""
    c = F.edge_case(cam_size)
    prob = c["prob"]
    pipe = _pipeline(c)
    info = pipe.fill_plan().info()
    assert (info["C"], info["W"], info["max_cam_list"], info["max_pt_list"]) == (F.C, F.W, 2 * F.C + 3, 7)
    exp = F.blockwise_expected(prob.num_pts, prob.num_cams, cam_size, prob.obs_cam, prob.obs_pt, c["Jc"], c["Jp"],
                               c["res"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=21 + cam_size)
    inputs = (c["Jc"], c["Jp"], c["res"])
    lay = c["lay"]
    alone = np.concatenate([3 * (prob.num_pts - 1) + np.arange(3),
                            3 * prob.num_pts + cam_size * (prob.num_cams - 1) + np.arange(cam_size)])
    mine = np.isin(lay["rows"], alone) | np.isin(lay["cols"], alone)
    assert mine.any() and not exp["Htouched"][mine].any()
    for lam in (0.0, 0.3):
        got, gotg = _run(pipe, inputs, dtype, lam, prior)
        F.check_fill(lay["diag"], dtype, exp, prior, got, gotg, lam, ("edges", cam_size, lam))
        _bitwise_the_model(pipe, c, inputs, dtype, lam, prior, got, gotg, ("edges", cam_size, lam))
        if lam == 0.0:
            assert bitwise_equal(got[mine], prior[0][mine])
        else:
            assert not bitwise_equal(got[lay["diag"][alone]], prior[0][lay["diag"][alone]])
        nog, none = _run(pipe, inputs, dtype, lam, prior, with_grad=False, twice=False)
        assert none is None and bitwise_equal(nog, got), "grad = None changed data"


@DTYPES
@pytest.mark.parametrize("cam_size", [9, 6])
def test_no_observations_damps_the_prior_only_or_writes_nothing(cam_size, dtype):
    """numObs = 0: with lambda = 0 nothing is written (negative zeros on the diagonal survive); with lambda = 0.3
    every diagonal entry is damped and no other word changes -- bitwise the model's fused damping"""
    c = R.fill_case("30x8", cam_size)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=5)
    diag = c["lay"]["diag"]
    prior[0][diag[::5]] = -0.0
    pipe = _pipeline(c, (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))
    assert pipe.fill_plan().info()["kept"] == 0
    empty = (np.zeros((0, 2, cam_size)), np.zeros((0, 2, 3)), np.zeros((0, 2)))
    got, gotg = _run(pipe, empty, dtype, 0.0, prior)
    assert bitwise_equal(got, prior[0]) and bitwise_equal(gotg, prior[1])
    got, gotg = _run(pipe, empty, dtype, 0.3, prior)
    want = prior[0].copy()
    F.damp(want, diag, 0.3, dtype)
    assert bitwise_equal(got, want) and bitwise_equal(gotg, prior[1])
    eps = np.finfo(dtype).eps
    h = prior[0][diag].astype(L)
    assert np.all(np.abs(got[diag].astype(L) - (h * (1 + L(0.3)) + L(3e-4))) <= 4 * eps * (np.abs(h) * 1.3 + 3e-4))
    # on the output of a fill, lambda = 0 with no observations leaves every bit
    full = _pipeline(c)
    filled = _run(full, (c["Jc"], c["Jp"], c["res"]), dtype, 0.0, prior, twice=False)
    again = _run(pipe, empty, dtype, 0.0, list(filled), twice=False)
    assert bitwise_equal(again[0], filled[0]) and bitwise_equal(again[1], filled[1])


@DTYPES
@pytest.mark.parametrize("cam_size", [9, 6])
def test_out_of_range_observations_give_the_bits_of_the_clean_list(cam_size, dtype):
    """the nine out-of-range observations of the atomic fill's test, mixed into the 30x8 list with Jacobians of
    their own: data and grad are bitwise those of the list without them"""
    c = R.fill_case("30x8", cam_size)
    oc, op, Jc, Jp, res, skipped = F.with_bad_observations(c)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=13)
    dirty, clean = _pipeline(c, (oc, op)), _pipeline(c)
    assert dirty.fill_plan().info()["skipped"] == 9
    for lam in (0.0, 0.3):
        got, gotg = _run(dirty, (Jc, Jp, res), dtype, lam, prior)
        want, wantg = _run(clean, (c["Jc"], c["Jp"], c["res"]), dtype, lam, prior, twice=False)
        assert bitwise_equal(got, want) and bitwise_equal(gotg, wantg)
        F.check_fill(c["lay"]["diag"], dtype, exp, prior, got, gotg, lam, ("out of range", cam_size, lam))


@DTYPES
@pytest.mark.parametrize("cam_size", [9, 6])
@pytest.mark.parametrize("name", R.FILL_SCENES)
def test_ordered_and_atomic_fill_agree_within_the_sum_of_their_bounds(name, cam_size, dtype):
    c = R.fill_case(name, cam_size)
    exp = R.expected_fill(c["ne"], c["lay"], dtype)
    prior = R.prior_for(exp, dtype, seed=2)
    pipe = _pipeline(c)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dt).reshape(-1)
    pipe.Jc, pipe.Jp, pipe.res = dev(c["Jc"], torch.float64), dev(c["Jp"], torch.float64), dev(c["res"], torch.float64)
    diag = c["lay"]["diag"]
    for lam in (0.0, 0.3):
        Ha, ga, Ho, go = dev(prior[0], tdt), dev(prior[1], tdt), dev(prior[0], tdt), dev(prior[1], tdt)
        pipe.fill_hessian(Ha, ga, lam)
        pipe.fill_hessian_ordered(Ho, go, lam)
        torch.cuda.synchronize()
        Ha, ga, Ho, go = (t.cpu().numpy() for t in (Ha, ga, Ho, go))
        bound = exp["Hbound"].copy()
        if lam != 0:
            eps = L(np.finfo(dtype).eps)
            h = np.abs(prior[0][diag].astype(L) + exp["H"][diag])
            bound[diag] = bound[diag] * (1 + L(lam)) + 4 * eps * (h * (1 + L(lam)) + L(1e-3) * L(lam))
        assert np.all(np.abs(Ha.astype(L) - Ho.astype(L)) <= 2 * bound), (name, cam_size, lam)
        assert np.all(np.abs(ga.astype(L) - go.astype(L)) <= 2 * exp["gbound"]), (name, cam_size, lam)
        same = ~exp["Htouched"]
        if lam != 0:
            same[diag] = False
        assert bitwise_equal(Ha[same], Ho[same])


def test_device_lm_with_the_ordered_fill_converges_on_the_scene_of_the_lm_test():
    """the conditions of test_device_lm_converges_on_the_scene_of_the_lm_test (tests/test_bal_step_gpu.py), on
    its scene, with ordered_fill=True.  (Not asserted: identical histories of two runs -- factor() may itself
    add atomically on some plans; the claim is H and g.)"""
    import baspacho_amd as B
    import bal_step_ref as S
    prob = bal.synth_scene(14, 300, seed=3, perturb=2e-2)
    sizes, ss, ranges = bal.bal_structure(prob, cam_size=6)
    sol = B.create_solver(B.Settings(), sizes, ss, ranges)
    cost0 = bal.total_cost(prob)
    lines = []
    out, hist = bal.lm_optimize_device(prob, sol, max_iters=25, log=lines.append, ordered_fill=True)
    cost1 = bal.total_cost(out)
    print("\n".join(lines))
    assert cost1 < 0.02 * cost0, (cost0, cost1, hist)
    assert cost1 < 2.0 * S.noise_floor(len(prob.obs_cam)), (cost1, len(prob.obs_cam))
    assert len([h for h in hist if h[1] <= h[0]]) >= 3
    assert len(lines) == len(hist) and abs(hist[0][0] - cost0) <= 1e-9 * cost0
    n = len(prob.obs_cam)
    dev = bal.DevicePipeline(out, sol, param="se3").cost().item()
    assert abs(dev - cost1) <= (n + 2) * S.EPS * cost1
    assert np.all(np.linalg.norm(out.cams[:, 0:3], axis=1) <= np.pi) and np.array_equal(out.cams[:, 6:9], prob.cams[:, 6:9])


def test_ordered_fill_runs_on_the_solvers_stream():
    """the pattern of test_pipeline_runs_on_the_solvers_stream (tests/test_bal_edges_gpu.py): with tens of ms of
    matmuls queued on a side stream s and then the copies that bring the true Jacobians into buffers that held
    NaN, the ordered fill must run after them on s.  On the null stream it would read the NaN.  The plan's
    tables were uploaded by an earlier call, so nothing in the call under test waits for the device."""
    c = R.fill_case("16x400", 9)
    sol = c["sol"]
    lam, dev = 0.3, "cuda"
    pipe = _pipeline(c)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(-1)
    true = [up(c["Jc"]), up(c["Jp"]), up(c["res"])]
    pipe.Jc, pipe.Jp, pipe.res = (t.clone() for t in true)

    def buffers():
        return (torch.zeros(sol.dataSize(), dtype=torch.float64, device=dev),
                torch.zeros(sol.order(), dtype=torch.float64, device=dev))
    H0, g0 = buffers()
    pipe.fill_hessian_ordered(H0, g0, lam)
    torch.cuda.synchronize()
    for t in (pipe.Jc, pipe.Jp, pipe.res):
        t.fill_(float("nan"))
    H, g = buffers()
    A = torch.randn(8192, 8192, dtype=torch.float64, device=dev)
    Cm = torch.empty_like(A)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    sol.setStream(s)
    try:
        with torch.cuda.stream(s):
            for _ in range(4):
                torch.matmul(A, A, out=Cm)
            for t, src in zip((pipe.Jc, pipe.Jp, pipe.res), true):
                t.copy_(src)
            pipe.fill_hessian_ordered(H, g, lam)
        s.synchronize()
    finally:
        sol.setStream(None)
    torch.cuda.synchronize()
    assert not torch.isnan(H).any() and not torch.isnan(g).any(), "the fill read the buffers before the copies on s"
    assert torch.equal(H, H0) and torch.equal(g, g0)
    # an explicit stream= overrides the solver's
    H2, g2 = buffers()
    for t in (pipe.Jc, pipe.Jp, pipe.res):
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.matmul(A, A, out=Cm)
        for t, src in zip((pipe.Jc, pipe.Jp, pipe.res), true):
            t.copy_(src)
        pipe.fill_hessian_ordered(H2, g2, lam, stream=s)
    s.synchronize()
    assert torch.equal(H2, H0) and torch.equal(g2, g0)
    del A, Cm
    torch.cuda.empty_cache()
