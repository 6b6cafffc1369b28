"""The device LM step of the BAL pipeline (csrc/bal_pipeline.hip through baspacho_amd/bal.py) against the
independent reference of tests/bal_step_ref.py, on framed buffers.

Residual kernels: every case of bal_ref.LIN_CASES in both parameterisations at bal_ref.LIN_BOUND.  Loss: rho
and the scaled words within LOSS_BOUND = 1.8e-15 relative of mpmath (8 x the float64 host model's worst error,
tests/test_bal_step_cpu.py), observations of weight 1 bitwise intact.  Sum: bitwise the numpy restatement of
the documented order.  Retraction: R(w_out) and t_out within STEP_BOUND_R = 2.7e-15 / STEP_BOUND_T = 1.3e-15
of the mpmath retraction from rotation matrices; points and bal9 cameras bitwise numpy.  End to end:
lm_optimize_device meets the conditions of the existing LM test, and on a scene with 5 % gross outliers the
robust losses reach what the trivial loss cannot."""
import ctypes

import numpy as np
import pytest
import torch

import baspacho_amd as B
import bal_ref as R
import bal_step_ref as S
from baspacho_amd import bal
from buffer_edges import Frame, framed, is_sentinel, bitwise_equal

pytestmark = pytest.mark.gpu
A = 2.0                                   # the loss size of every loss test: a and a^2 are exact
LOSS_COUNTS = R.OBS_COUNTS + (515,)       # and two full tiles of 256 observations plus three


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64).view(np.float64)


def _as_i64(t):
    return t.view(torch.int64)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


_SOLVERS = {}


def _solver(name, cam_size):
    """(problem, solver) of a bal_ref linearisation case or fill scene, built once"""
    if (name, cam_size) not in _SOLVERS:
        if name in R.LIN_CASES:
            prob, ranges = R.lin_problem(name), None
        else:
            prob, ranges = R._fill_problem(name)
        sizes, ss, auto = bal.bal_structure(prob, cam_size=cam_size)
        _SOLVERS[name, cam_size] = (prob, B.create_solver(B.Settings(), sizes, ss, auto if ranges is None else ranges))
    return _SOLVERS[name, cam_size]


def _pipe(name, param, loss=None):
    prob, sol = _solver(name, 9 if param == "bal9" else 6)
    return bal.DevicePipeline(prob, sol, param=param, loss=loss)


def _se3_solver(prob):
    sizes, ss, ranges = bal.bal_structure(prob, cam_size=6)
    return B.create_solver(B.Settings(), sizes, ss, ranges)


# ---- 1: residual kernels ---------------------------------------------------------------------------------
LIN_RUNS = [("generic", n) for n in R.OBS_COUNTS] + [(name, None) for name in R.LIN_CASES if name != "generic"]


@pytest.mark.parametrize("name,count", LIN_RUNS, ids=["%s-%s" % r for r in LIN_RUNS])
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_residuals_against_the_reference(param, name, count):
    prob = R.lin_problem(name)
    n = len(prob.obs_cam) if count is None else count
    ref = tuple(a[:n] for a in R.lin_reference(name, param))
    fin = framed(np.float64, [_i64(prob.obs_cam[:n]), _i64(prob.obs_pt[:n]), prob.obs_xy[:n], prob.cams, prob.pts])
    fout = Frame([2 * n], np.float64)
    pipe = _pipe(name, param)
    pipe.obs_cam, pipe.obs_pt, pipe.obs_xy = _as_i64(fin.view(0)), _as_i64(fin.view(1)), fin.view(2)
    pipe.cams, pipe.pts, pipe.n_obs = fin.view(3), fin.view(4), n
    got = pipe.residuals(out=fout.view(0))
    torch.cuda.synchronize()
    assert got.data_ptr() == fout.view(0).data_ptr()
    fout.assert_intact(what="residual output")
    fin.assert_intact(read_only=range(5), what="residual inputs")
    res = fout.host(0)
    assert not is_sentinel(res).any(), "an output word was not written"
    eres, _ = R.lin_errors((res, ref[1], ref[2]), ref)
    print("%s %s n=%d: residual %.2e (bound %.1e)" % (param, name, n, eres, R.LIN_BOUND))
    assert eres <= R.LIN_BOUND, eres
    if name == "special" and param == "se3":
        res = res.reshape(n, 2)
        for o, z in R.SPECIAL_Z.items():
            assert bitwise_equal(res[o], np.array([25.0, 0.0])) == (z > 0.01)
    # explicit parameters override the pipeline's own
    pipe.cams, pipe.pts = None, None
    again = pipe.residuals(fin.view(3), fin.view(4))
    torch.cuda.synchronize()
    assert bitwise_equal(again.cpu().numpy(), fout.host(0))


@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_no_observations_launch_nothing(param):
    """n = 0: residuals and loss of an empty problem write nothing; the sum writes +0.0"""
    pipe = _pipe("generic", param, loss=("huber", A))
    fr = Frame([4, 4, 4, 4, 4], np.float64)
    pipe.n_obs = 0
    pipe.res, pipe.Jc, pipe.Jp, pipe.rho = fr.view(0)[:0], fr.view(1)[:0], fr.view(2)[:0], fr.view(3)[:0]
    pipe.residuals(out=fr.view(0)[:0])
    pipe.apply_loss()
    out = pipe.cost_linearized(out=fr.view(4)[0:1])
    torch.cuda.synchronize()
    fr.assert_intact(what="empty problem")
    assert all(is_sentinel(fr.host(k)).all() for k in range(4))
    got = fr.host(4)
    assert bitwise_equal(got[:1], np.array([0.0])) and is_sentinel(got[1:]).all() and float(out) == 0.0


# ---- 2: loss kernel --------------------------------------------------------------------------------------
def _loss_call(pipe, n, cs, kind, a, res, Jc, Jp, rho):
    return pipe.lib.bsp_bal_loss_f64(ctypes.c_int64(n), ctypes.c_int32(cs), ctypes.c_int32(kind), ctypes.c_double(a),
                                     _ptr(res), _ptr(Jc), _ptr(Jp), _ptr(rho), ctypes.c_void_p(0))


def _loss_inputs(n, cs, seed):
    res, fixed = S.loss_cases(A, n, seed=seed)
    rng = np.random.default_rng(seed + 50)
    Jc, Jp = rng.uniform(-50, 50, (n, 2 * cs)), rng.uniform(-50, 50, (n, 6))
    Jc[fixed], Jp[fixed] = 0.0, 0.0            # the behind-the-camera row: (25, 0) and zero Jacobians
    return res, Jc, Jp


@pytest.mark.parametrize("n", LOSS_COUNTS)
@pytest.mark.parametrize("kind", ["trivial", "huber", "cauchy"])
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_loss_against_the_reference(param, kind, n):
    cs = 9 if param == "bal9" else 6
    res, Jc, Jp = _loss_inputs(n, cs, S.KINDS[kind])
    fio = framed(np.float64, [res, Jc, Jp])
    frho = Frame([n], np.float64)
    pipe = _pipe("generic", param, loss=None if kind == "trivial" else (kind, A))
    pipe.res, pipe.Jc, pipe.Jp, pipe.rho, pipe.n_obs = fio.view(0), fio.view(1), fio.view(2), frho.view(0), n
    pipe.apply_loss()
    torch.cuda.synchronize()
    assert pipe.rho.data_ptr() == frho.view(0).data_ptr()
    fio.assert_intact(what="loss operands")
    frho.assert_intact(what="rho")
    rho = frho.host(0)
    assert not is_sentinel(rho).any(), "a word of rho was not written"
    after = [fio.host(k).reshape(n, -1) for k in range(3)]
    e_rho, e_w = S.loss_errors(kind, A, res, rho, list(zip((res, Jc, Jp), after)))
    print("%s %s n=%d: rho %.2e words %.2e (bound %.1e)" % (param, kind, n, e_rho, e_w, S.LOSS_BOUND))
    assert e_rho <= S.LOSS_BOUND and e_w <= S.LOSS_BOUND, (e_rho, e_w)
    unit = S.unit_weight(kind, A, res)
    for before, got in zip((res, Jc, Jp), after):
        assert bitwise_equal(got[unit], before[unit]), "an observation of weight 1 was rewritten"
    if kind != "trivial" and n > 8:
        assert not bitwise_equal(after[0][~unit], res[~unit])
    # only rho: the candidate's cost.  res is bitwise intact, rho the same bits
    fres = framed(np.float64, [res])
    frho2 = Frame([n], np.float64)
    assert _loss_call(pipe, n, cs, S.KINDS[kind], A, fres.view(0), None, None, frho2.view(0)) == 0
    torch.cuda.synchronize()
    fres.assert_intact(read_only=[0], what="res with NULL Jacobians")
    frho2.assert_intact(what="rho with NULL Jacobians")
    assert bitwise_equal(frho2.host(0), rho)


@pytest.mark.parametrize("kind,a", [(1, 0.0), (2, -2.0), (1, float("nan")), (2, float("inf")), (3, 2.0), (-1, 2.0)])
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_loss_refuses_bad_arguments_and_writes_nothing(param, kind, a):
    cs, n = (9 if param == "bal9" else 6), 65
    res, Jc, Jp = _loss_inputs(n, cs, 7)
    fio = framed(np.float64, [res, Jc, Jp])
    frho = Frame([n], np.float64)
    pipe = _pipe("generic", param)
    assert _loss_call(pipe, n, cs, kind, a, fio.view(0), fio.view(1), fio.view(2), frho.view(0)) != 0
    assert len(pipe.lib.bsp_last_error()) > 0
    torch.cuda.synchronize()
    fio.assert_intact(read_only=range(3), what="refused loss call")
    frho.assert_intact(what="refused loss call")
    assert is_sentinel(frho.host(0)).all()
    if kind in (1, 2) and not a > 0:
        with pytest.raises(RuntimeError):
            p2 = _pipe("generic", param, loss=("huber" if kind == 1 else "cauchy", a))
            p2.linearize()
            p2.apply_loss()


# ---- 3: sum ------------------------------------------------------------------------------------------------
SUM_COUNTS = (0, 1, S.SUM_CHUNK - 1, S.SUM_CHUNK, S.SUM_CHUNK + 1, S.SUM_CHUNK * S.SUM_WIDTH + 1)


@pytest.mark.parametrize("n", SUM_COUNTS)
def test_sum_is_bitwise_the_documented_order(n):
    rng = np.random.default_rng(n % 1000 + 3)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    pipe = _pipe("generic", "se3")
    need = int(pipe.lib.bsp_bal_sum_scratch_len(ctypes.c_int64(n)))
    assert need == -(-n // S.SUM_CHUNK)
    fx = framed(np.float64, [x])
    want = S.sum_model(x, 0.5)
    seen = []
    for _ in range(2):
        fs, fo = Frame([need], np.float64), Frame([3], np.float64)
        rc = pipe.lib.bsp_bal_sum_f64(ctypes.c_int64(n), _ptr(fx.view(0)), ctypes.c_double(0.5), _ptr(fs.view(0)),
                                      _ptr(fo.view(0)), ctypes.c_void_p(0))
        assert rc == 0, pipe.lib.bsp_last_error()
        torch.cuda.synchronize()
        fx.assert_intact(read_only=[0], what="sum input")
        fs.assert_intact(what="sum scratch")
        fo.assert_intact(what="sum output")
        out = fo.host(0)
        assert is_sentinel(out[1:]).all(), "a word of out beyond [0] was written"
        seen.append(out[:1])
    assert bitwise_equal(seen[0], seen[1]), "two runs differ"
    assert bitwise_equal(seen[0], np.array([want])), (n, seen[0][0], want)
    if n == 0:
        assert not np.signbit(seen[0][0])


# ---- 4: retraction -----------------------------------------------------------------------------------------
def _internal_offsets(sol, num_params):
    perm = sol.paramToSpan()
    return np.array([sol.spanVectorOffset(int(perm[p])) for p in range(num_params)], dtype=np.int64)


def _run_apply_step(prob, sol, param, step):
    """apply_step on framed buffers: (cams_out (nc, 9), pts_out (npt, 3)), frames and inputs checked"""
    fin = framed(np.float64, [prob.cams, prob.pts, step])
    pipe = bal.DevicePipeline(prob, sol, param=param)
    pipe.cams, pipe.pts = fin.view(0), fin.view(1)
    cams, pts = pipe.apply_step(fin.view(2))
    torch.cuda.synchronize()
    fin.assert_intact(read_only=range(3), what="apply_step inputs")
    assert cams.data_ptr() != fin.view(0).data_ptr() and pts.data_ptr() != fin.view(1).data_ptr()
    return cams.cpu().numpy().reshape(-1, 9), pts.cpu().numpy().reshape(-1, 3)


def _step_scene():
    """STEP_CASES as the cameras of a small scene in which every camera sees every point"""
    if "steps" not in _SOLVERS:
        nc, npt = len(S.STEP_CAMS), 7
        pts = np.random.default_rng(4).uniform(-2, 2, (npt, 3))
        oc, op = np.repeat(np.arange(nc), npt), np.tile(np.arange(npt), nc)
        prob = bal.BalProblem(S.STEP_CAMS.copy(), pts, oc, op, np.zeros((len(oc), 2)))
        sizes, ss, ranges = bal.bal_structure(prob, cam_size=6)
        _SOLVERS["steps"] = (prob, B.create_solver(B.Settings(), sizes, ss, ranges))
    return _SOLVERS["steps"]


def test_se3_retraction_against_the_reference():
    prob, sol = _step_scene()
    npt, nc = prob.num_pts, prob.num_cams
    off = _internal_offsets(sol, npt + nc)
    dpt = 1e-2 * np.random.default_rng(8).standard_normal((npt, 3))
    step = np.zeros(sol.order())
    step[off[:npt, None] + np.arange(3)] = dpt
    step[off[npt:, None] + np.arange(6)] = S.STEP_STEPS
    # outputs on a frame too: every word written, nothing beside them
    fin = framed(np.float64, [prob.cams, prob.pts, step])
    fout = Frame([9 * nc, 3 * npt], np.float64)
    pipe = bal.DevicePipeline(prob, sol, param="se3")
    rc = pipe.lib.bsp_bal_apply_step_se3_f64(sol._h, ctypes.c_int64(npt), ctypes.c_int64(nc), _ptr(fin.view(0)),
                                             _ptr(fin.view(1)), _ptr(fin.view(2)), _ptr(fout.view(0)),
                                             _ptr(fout.view(1)), ctypes.c_void_p(0))
    assert rc == 0, pipe.lib.bsp_last_error()
    torch.cuda.synchronize()
    fin.assert_intact(read_only=range(3), what="apply_step inputs")
    fout.assert_intact(what="apply_step outputs")
    cams, pts = fout.host(0).reshape(nc, 9), fout.host(1).reshape(npt, 3)
    assert not is_sentinel(cams).any() and not is_sentinel(pts).any(), "an output word was not written"
    eR, eT = S.step_errors(S.STEP_CAMS, S.STEP_STEPS, cams)
    for name, a, b in zip(S.STEP_NAMES, eR, eT):
        print("%-45s R %.2e  t %.2e" % (name, a, b))
    print("worst R %.2e (bound %.1e)  t %.2e (bound %.1e)" % (eR.max(), S.STEP_BOUND_R, eT.max(), S.STEP_BOUND_T))
    assert eR.max() <= S.STEP_BOUND_R and eT.max() <= S.STEP_BOUND_T, (eR.max(), eT.max())
    assert np.all(np.linalg.norm(cams[:, 0:3], axis=1) <= np.pi * (1 + 4 * S.EPS))
    assert bitwise_equal(cams[:, 6:9], S.STEP_CAMS[:, 6:9]), "the calibration is copied"
    assert bitwise_equal(pts, prob.pts - dpt)
    # the method returns the same bits as new tensors
    cams2, pts2 = _run_apply_step(prob, sol, "se3", step)
    assert bitwise_equal(cams2, cams) and bitwise_equal(pts2, pts)


@pytest.mark.parametrize("name", ["40x6", "37x5", "30x8", "9x9"])
@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_retraction_gathers_the_step_through_the_permutation(param, name):
    """scenes in which the solver's order is not the caller's: a step whose value encodes its internal index
    (index / 1024, exact) must reach parameter p from spanVectorOffset(paramToSpan()[p])"""
    cs = 9 if param == "bal9" else 6
    prob, sol = _solver(name, cs)
    npt, nc = prob.num_pts, prob.num_cams
    off = _internal_offsets(sol, npt + nc)
    caller = np.concatenate([3 * np.arange(npt), 3 * npt + cs * np.arange(nc)])
    assert not np.array_equal(off, caller), "the ordering is the identity: the scene checks nothing"
    step = np.arange(sol.order(), dtype=np.float64) / 1024.0
    cams, pts = _run_apply_step(prob, sol, param, step)
    assert bitwise_equal(pts, prob.pts - step[off[:npt, None] + np.arange(3)])
    cam_step = step[off[npt:, None] + np.arange(cs)]
    if param == "bal9":
        assert bitwise_equal(cams, prob.cams - cam_step)
    else:
        eR, eT = S.step_errors(prob.cams, cam_step, cams)
        assert eR.max() <= S.STEP_BOUND_R and eT.max() <= S.STEP_BOUND_T, (eR.max(), eT.max())
        assert bitwise_equal(cams[:, 6:9], prob.cams[:, 6:9])


@pytest.mark.parametrize("param", ["bal9", "se3"])
def test_retraction_refuses_a_solver_of_the_wrong_camera_width(param):
    cs = 9 if param == "bal9" else 6
    prob, sol = _solver("30x8", 15 - cs)    # the other width
    fin = framed(np.float64, [prob.cams, prob.pts, np.ones(sol.order())])
    fout = Frame([9 * prob.num_cams, 3 * prob.num_pts], np.float64)
    lib = bal.DevicePipeline(prob, sol, param=param).lib
    fn = lib.bsp_bal_apply_step_f64 if param == "bal9" else lib.bsp_bal_apply_step_se3_f64
    rc = fn(sol._h, ctypes.c_int64(prob.num_pts), ctypes.c_int64(prob.num_cams), _ptr(fin.view(0)), _ptr(fin.view(1)),
            _ptr(fin.view(2)), _ptr(fout.view(0)), _ptr(fout.view(1)), ctypes.c_void_p(0))
    assert rc != 0 and len(lib.bsp_last_error()) > 0
    torch.cuda.synchronize()
    fin.assert_intact(read_only=range(3), what="refused apply_step")
    fout.assert_intact(what="refused apply_step")
    assert is_sentinel(fout.host(0)).all() and is_sentinel(fout.host(1)).all()
    with pytest.raises(RuntimeError):
        bal.DevicePipeline(prob, sol, param=param).apply_step(fin.view(2))


# ---- cost ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [None, ("huber", A), ("cauchy", A)], ids=["trivial", "huber", "cauchy"])
def test_cost_against_the_reference(loss):
    """cost() = 0.5 sum rho from the residual-only kernel against mpmath.  Bound: the residuals are within
    LIN_BOUND (scaled by |projection| + |xy|), rho' <= 1 turns an error d in s = |r|^2 into at most d in rho,
    rho itself is within LOSS_BOUND, and the sum of n positive terms within (n + 2) eps.  cost_linearized()
    after linearize() + apply_loss() is the same function of the parameters, to the same bound."""
    prob = R.lin_problem("generic")
    pipe = _pipe("generic", "se3", loss=loss)
    kind, a = (0, 1.0) if loss is None else (S.KINDS[loss[0]], loss[1])
    want, terms = S.cost_mp(prob, kind, a)
    ref = R.lin_reference("generic", "se3")
    scale = np.abs(ref[3]).max(axis=1) + np.abs(ref[3] - ref[0]).max(axis=1)
    dr = R.LIN_BOUND * scale
    bound = 0.5 * float(np.sum(2 * terms[:, 0] * dr + 2 * dr * dr + S.LOSS_BOUND * terms[:, 1])) \
        + (len(scale) + 2) * S.EPS * want
    got = pipe.cost()
    assert got.dim() == 0 and got.is_cuda
    pipe.linearize()
    res_before = pipe.res.clone()
    pipe.apply_loss()
    lin = pipe.cost_linearized()
    assert pipe.cost(pipe.cams, pipe.pts).item() == got.item()
    print("%s: cost %.17g linearised %.17g reference %.17g bound %.2e" % (loss, got.item(), lin.item(), want, bound))
    assert abs(got.item() - want) <= bound and abs(lin.item() - want) <= bound
    assert (loss is None) == torch.equal(pipe.res, res_before)


# ---- 5, 6: end to end ------------------------------------------------------------------------------------
def test_device_lm_converges_on_the_scene_of_the_lm_test():
    prob = bal.synth_scene(14, 300, seed=3, perturb=2e-2)
    sol = _se3_solver(prob)
    cost0 = bal.total_cost(prob)
    lines = []
    out, hist = bal.lm_optimize_device(prob, sol, max_iters=25, log=lines.append)
    cost1 = bal.total_cost(out)
    print("\n".join(lines))
    assert cost1 < 0.02 * cost0, (cost0, cost1, hist)
    assert cost1 < 2.0 * S.noise_floor(len(prob.obs_cam)), (cost1, len(prob.obs_cam))
    assert len([h for h in hist if h[1] <= h[0]]) >= 3
    assert len(lines) == len(hist) and abs(hist[0][0] - cost0) <= 1e-9 * cost0
    n = len(prob.obs_cam)
    dev = bal.DevicePipeline(out, sol, param="se3").cost().item()
    print("cost() %.17g total_cost %.17g rel %.2e (bound %.2e)" % (dev, cost1, abs(dev - cost1) / cost1, (n + 2) * S.EPS))
    assert abs(dev - cost1) <= (n + 2) * S.EPS * cost1
    assert np.all(np.linalg.norm(out.cams[:, 0:3], axis=1) <= np.pi) and np.array_equal(out.cams[:, 6:9], prob.cams[:, 6:9])


def test_device_lm_with_robust_losses_on_the_outlier_scene():
    """5 % of the observations off by 40 .. 80 px.  Conditions (not measurements; the host LM of bal_step_ref
    meets them at 132 x, 0.076 x and 0.47 x): the trivial loss ends above 20 x the inlier noise floor, Huber(2)
    below 0.2 x the trivial result, Cauchy(2) below 2 x the floor."""
    prob, inlier = S.outlier_scene(3)
    sol = _se3_solver(prob)
    floor = S.noise_floor(int(inlier.sum()))
    end = {}
    for loss in (None, ("huber", 2.0), ("cauchy", 2.0)):
        out, hist = bal.lm_optimize_device(prob, sol, loss=loss)
        end[loss and loss[0]] = S.inlier_cost(out, inlier)
        print("%s: inlier cost %.1f = %.2f x floor after %d iterations" % (loss, end[loss and loss[0]],
                                                                          end[loss and loss[0]] / floor, len(hist)))
        assert all(np.isfinite(h).all() for h in hist)
    assert end[None] > 20 * floor, end
    assert end["huber"] < 0.2 * end[None], end
    assert end["cauchy"] < 2 * floor, end
