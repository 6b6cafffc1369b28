"""Bundle-adjustment-at-large caller pipeline: BAL text files, the solver structure the reference's
BAL_bench builds from them, and the device-side linearisation / Hessian assembly.

Mirrors benchmarking/BaAtLarge.cpp:81-182 (Data::load: header `numCams numPts numObs`, one line
`cam pt x y` per observation, 9 numbers per camera -- Rodrigues rotation, translation, f, k1, k2 --
3 per point; same error behaviour: a bad index or a short file raises), :184-230 (save),
BaAtLargeBench.cpp:44-73 (structure: points first, size 3, cameras after, size 9, one block per
observation, sparse elimination range {0, numPts}) and BaAtLargeOptimizer.cpp:100-131 (computeStep:
Hessian / gradient assembly through the accessor + LM damping), the last on the GPU through
Solver::deviceAccessor() (csrc/bal_pipeline.hip)."""
import bz2
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .testing import structure_from_pairs


@dataclass
class BalProblem:
    cams: np.ndarray      # (numCams, 9): r(3), t(3), f, k1, k2
    pts: np.ndarray       # (numPts, 3)
    obs_cam: np.ndarray   # (numObs,) int64
    obs_pt: np.ndarray    # (numObs,) int64
    obs_xy: np.ndarray    # (numObs, 2)

    @property
    def num_cams(self):
        return len(self.cams)

    @property
    def num_pts(self):
        return len(self.pts)


def load_bal(path):
    """Data::load (BaAtLarge.cpp:81-182); .bz2 files (as the BAL site ships them) are accepted"""
    try:
        if str(path).endswith(".bz2"):
            with bz2.open(path, "rt") as f:
                tok = np.array(f.read().split(), dtype=np.float64)
        else:
            tok = np.fromfile(path, dtype=np.float64, sep=" ")
    except OSError as e:
        raise RuntimeError("Cannot open file `%s`" % path) from e
    if len(tok) < 3:
        raise RuntimeError("Cannot open file `%s`" % path)
    nc, npt, nobs = (int(v) for v in tok[:3])
    need = 3 + 4 * nobs + 9 * nc + 3 * npt
    body = tok[3:]
    if len(tok) < 3 + 4 * nobs:
        raise RuntimeError("File error loading %dth observation!" % ((len(tok) - 3) // 4))
    obs = body[:4 * nobs].reshape(nobs, 4)
    cam_idx, pt_idx = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    bad = np.nonzero((cam_idx >= nc) | (cam_idx < 0))[0]
    if len(bad):
        raise RuntimeError("Error loading %dth observation, invalid camera index: %d"
                           % (bad[0], cam_idx[bad[0]]))
    bad = np.nonzero((pt_idx >= npt) | (pt_idx < 0))[0]
    if len(bad):
        raise RuntimeError("Error loading %dth observation, invalid point index: %d"
                           % (bad[0], pt_idx[bad[0]]))
    if len(tok) < 3 + 4 * nobs + 9 * nc:
        raise RuntimeError("File error loading %dth camera!" % ((len(tok) - 3 - 4 * nobs) // 9))
    if len(tok) < need:
        raise RuntimeError("File error loading %dth point!" % ((len(tok) - 3 - 4 * nobs - 9 * nc) // 3))
    cams = body[4 * nobs:4 * nobs + 9 * nc].reshape(nc, 9).copy()
    pts = body[4 * nobs + 9 * nc:4 * nobs + 9 * nc + 3 * npt].reshape(npt, 3).copy()
    return BalProblem(cams, pts, cam_idx, pt_idx, obs[:, 2:4].copy())


def save_bal(path, prob):
    """Data::save (BaAtLarge.cpp:184-230): the same text layout, %.16e precision"""
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (prob.num_cams, prob.num_pts, len(prob.obs_cam)))
        for c, p, (x, y) in zip(prob.obs_cam, prob.obs_pt, prob.obs_xy):
            f.write("%d %d %.16e %.16e\n" % (c, p, x, y))
        for v in prob.cams.reshape(-1):
            f.write("%.16e\n" % v)
        for v in prob.pts.reshape(-1):
            f.write("%.16e\n" % v)


def bal_structure(prob, cam_size=9):
    """(paramSizes, SparseStructure, sparseElimRanges) as testSolvers builds them
    (BaAtLargeBench.cpp:44-73): points first, then cameras; block (numPts + cam, pt) per observation.
    cam_size = 9: the camera blocks of BAL_bench (all parameters of a BAL file); cam_size = 6: the
    blocks of the LM optimizer BAL_opt (SE3 tangent, BaAtLargeOptimizer.cpp:33-52)"""
    npt, nc = prob.num_pts, prob.num_cams
    sizes = np.concatenate([np.full(npt, 3, dtype=np.int64), np.full(nc, cam_size, dtype=np.int64)])
    key = np.unique(prob.obs_pt * nc + prob.obs_cam)   # duplicate observations share a block
    ss = structure_from_pairs(npt + nc, npt + key % nc, key // nc)
    return sizes, ss, [0, npt]


def project(cams, pts):
    """the BAL camera model on arrays: p = -P.xy / P.z with P = R(r) X + t, then f (1 + k1 r^2 +
    k2 r^4) p (numpy; used to synthesise observations)"""
    w, t = cams[:, 0:3], cams[:, 3:6]
    th = np.linalg.norm(w, axis=1, keepdims=True)
    k = w / np.maximum(th, 1e-300)
    c, s = np.cos(th), np.sin(th)
    P = pts * c + np.cross(k, pts) * s + k * (np.sum(k * pts, axis=1, keepdims=True)) * (1 - c) + t
    p = -P[:, :2] / P[:, 2:3]
    r2 = np.sum(p * p, axis=1, keepdims=True)
    return cams[:, 6:7] * (1 + r2 * (cams[:, 7:8] + cams[:, 8:9] * r2)) * p


def synth_scene(num_cams=12, num_pts=200, mean_track=4, seed=3, noise=0.5, perturb=1e-2):
    """a small geometrically consistent scene: cameras on an arc looking at a point cloud, pixel
    noise on the observations, parameters perturbed off the truth (so that an LM step has work)"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-0.6, 0.6, num_cams)
    cams = np.zeros((num_cams, 9))
    cams[:, 1] = ang                                   # rotation about y
    cams[:, 0] = 0.05 * rng.standard_normal(num_cams)
    cams[:, 3] = 2.0 * np.sin(ang)
    cams[:, 5] = -12.0 + rng.uniform(-0.5, 0.5, num_cams)   # scene in front of the camera (z < 0)
    cams[:, 6] = 800.0 + rng.uniform(-20, 20, num_cams)
    cams[:, 7] = 1e-2 * rng.standard_normal(num_cams)
    cams[:, 8] = 1e-4 * rng.standard_normal(num_cams)
    pts = rng.uniform(-2.0, 2.0, (num_pts, 3))
    oc, op = [], []
    for p in range(num_pts):
        k = int(min(num_cams, max(2, rng.poisson(mean_track))))
        c0 = rng.integers(0, num_cams)
        sel = np.unique(np.clip(c0 + rng.integers(-3, 4, size=k), 0, num_cams - 1))
        if len(sel) < 2:
            sel = np.array([c0, (c0 + 1) % num_cams])
        oc.extend(sel.tolist())
        op.extend([p] * len(sel))
    oc, op = np.array(oc, dtype=np.int64), np.array(op, dtype=np.int64)
    xy = project(cams[oc], pts[op]) + noise * rng.standard_normal((len(oc), 2))
    cams = cams + perturb * rng.standard_normal(cams.shape) * np.array([1, 1, 1, 1, 1, 1, 100, 1e-2, 1e-4])
    pts = pts + perturb * rng.standard_normal(pts.shape)
    return BalProblem(cams, pts, oc, op, xy)


def synth_scene_for(num_cams, num_pts, obs_cam, obs_pt, seed=3, noise=0.5, perturb=1e-2):
    """a geometrically consistent scene for a GIVEN observation list (e.g. the co-visibility of
    testing.gen_bal_synthetic at BAL-871 / BAL-1723 size): cameras on a wide arc around a point cloud,
    every listed observation projected through the BAL camera model + pixel noise, parameters
    perturbed off the truth.  Vectorised (no per-point loop); the Hessian J^T J of the result is a
    real bundle-adjustment Hessian, not a diagonally dominant mock."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-1.2, 1.2, num_cams)
    cams = np.zeros((num_cams, 9))
    cams[:, 1] = ang
    cams[:, 0] = 0.05 * rng.standard_normal(num_cams)
    cams[:, 3] = 2.0 * np.sin(ang)
    cams[:, 5] = -12.0 + rng.uniform(-0.5, 0.5, num_cams)
    cams[:, 6] = 800.0 + rng.uniform(-20, 20, num_cams)
    cams[:, 7] = 1e-2 * rng.standard_normal(num_cams)
    cams[:, 8] = 1e-4 * rng.standard_normal(num_cams)
    pts = rng.uniform(-2.0, 2.0, (num_pts, 3))
    oc = np.ascontiguousarray(obs_cam, dtype=np.int64)
    op = np.ascontiguousarray(obs_pt, dtype=np.int64)
    xy = project(cams[oc], pts[op]) + noise * rng.standard_normal((len(oc), 2))
    cams = cams + perturb * rng.standard_normal(cams.shape) * np.array([1, 1, 1, 1, 1, 1, 100, 1e-2, 1e-4])
    pts = pts + perturb * rng.standard_normal(pts.shape)
    return BalProblem(cams, pts, oc, op, xy)


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)


def so3_exp(w):
    th = float(np.linalg.norm(w))
    K = _skew(w)
    if th < 1e-10:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def so3_log(R):
    c = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-10:
        return 0.5 * v
    if np.pi - th < 1e-6:   # near pi: axis from the symmetric part
        A = 0.5 * (R + np.eye(3))
        ax = np.sqrt(np.maximum(np.diag(A), 0.0))
        k = int(np.argmax(ax))
        ax = A[:, k] / ax[k]
        return th * ax / np.linalg.norm(ax)
    return th / (2.0 * np.sin(th)) * v


def se3_exp(delta):
    """Sophus::SE3d::exp for delta = (translation part, rotation part): (R, t)"""
    u, w = np.asarray(delta[:3], dtype=np.float64), np.asarray(delta[3:], dtype=np.float64)
    th = float(np.linalg.norm(w))
    K = _skew(w)
    if th < 1e-10:
        V = np.eye(3) + 0.5 * K + K @ K / 6.0
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    return so3_exp(w), V @ u


def apply_step_se3(prob, step, solver):
    """applyStep of the reference's optimizer (BaAtLargeOptimizer.cpp:170-184): points -= step,
    T_W_C <- exp(-step) T_W_C; `step` is in the solver's internal order (paramToSpan /
    spanVectorOffset); cameras keep the BAL storage (Rodrigues rotation, translation).  Returns a
    new BalProblem."""
    out = BalProblem(prob.cams.copy(), prob.pts.copy(), prob.obs_cam, prob.obs_pt, prob.obs_xy)
    perm = solver.paramToSpan()
    ss = solver.skel()["spanStart"]
    npt = prob.num_pts
    pt_off = ss[perm[:npt]]
    out.pts -= step[pt_off[:, None] + np.arange(3)[None, :]]
    for i in range(prob.num_cams):
        o = int(ss[perm[npt + i]])
        Rd, td = se3_exp(-step[o:o + 6])
        R = so3_exp(prob.cams[i, 0:3])
        out.cams[i, 0:3] = so3_log(Rd @ R)
        out.cams[i, 3:6] = Rd @ prob.cams[i, 3:6] + td
    return out


def total_cost(prob):
    """computeCost (BaAtLargeOptimizer.cpp:54-63) with the reference's behind-the-camera rule"""
    w, t = prob.cams[prob.obs_cam, 0:3], prob.cams[prob.obs_cam, 3:6]
    X = prob.pts[prob.obs_pt]
    th = np.linalg.norm(w, axis=1, keepdims=True)
    k = w / np.maximum(th, 1e-300)
    P = X * np.cos(th) + np.cross(k, X) * np.sin(th) + k * np.sum(k * X, axis=1, keepdims=True) * (1 - np.cos(th)) + t
    bad = P[:, 2] > 0.01
    err = project(prob.cams[prob.obs_cam], X) - prob.obs_xy
    err[bad] = (25.0, 0.0)
    return 0.5 * float(np.sum(err * err))


def lm_optimize(prob, solver, max_iters=50, lam=1e-5, log=None):
    """the Levenberg-Marquardt loop of BAL_opt (BaAtLargeOptimizer.cpp:186-234), every numeric stage
    on the device: linearise (SE3 tangent) -> Hessian through deviceAccessor() -> factor -> solve ->
    exp-map update; same lambda schedule, same acceptance and convergence rules.  `solver` must have
    6-wide camera blocks (bal_structure(prob, cam_size=6)).  Returns (problem, cost history)."""
    import torch
    hist = []
    last_failed = last_ok = last_good = 0
    for i in range(max_iters):
        pipe = DevicePipeline(prob, solver, param="se3")
        pipe.linearize()
        cost = 0.5 * float((pipe.res * pipe.res).sum())
        H = torch.zeros(solver.dataSize(), dtype=torch.float64, device=pipe.res.device)
        g = torch.zeros(solver.order(), dtype=torch.float64, device=pipe.res.device)
        pipe.fill_hessian(H, g, lam)
        step = g.clone()
        solver.factor(H)
        solver.solve(H, step, solver.order(), 1)
        cand = apply_step_se3(prob, step.cpu().numpy(), solver)
        model_red = 0.5 * float(torch.dot(g, step))
        new_cost = total_cost(cand)
        bad, good = new_cost > cost, new_cost < cost * 0.999
        hist.append((cost, new_cost, lam))
        if log:
            log("[%d] cost %.3e -> %.3e lambda %.1e" % (i, cost, new_cost, lam))
        if bad:
            last_failed = i
            if lam > 1e8 or i > last_ok + 15:
                break
            lam *= 3
            continue
        prob = cand
        last_ok = i
        if good:
            last_good = i
        rel_red = (cost - new_cost) / model_red if model_red != 0 else 0.0
        if rel_red > 0.6:
            lam *= 0.6
        elif rel_red < 0.4:
            lam *= 1.3
        if i >= last_good + 3 and i >= last_failed + 3:
            break
    return prob, hist


def lm_optimize_device(prob, solver, max_iters=50, lam=1e-5, loss=None, log=None, ordered_fill=False):
    """lm_optimize with the whole iteration resident on the device: one DevicePipeline for the run, H, g,
    step, rho and the sum scratch reused, the candidate retracted (apply_step) and its cost evaluated
    (cost) by device kernels, and ONE device-to-host read per iteration, the 3-element tensor
    [cost, new_cost, 0.5 g.step] every decision is taken from.  Same lambda schedule, acceptance and
    stopping rules as lm_optimize, line for line.  loss: None, ("huber", a) or ("cauchy", a) -- the robust
    loss of the reference's optimizer (examples/SoftLoss.h; H += rho' J^T J, g += rho' J^T r, cost =
    rho / 2); the costs in the history are then robust costs.  `solver` must have 6-wide camera blocks.
    ordered_fill=True assembles H and g with fill_hessian_ordered (no atomics: the same bits on every run)
    instead of fill_hessian; nothing else changes.  Everything runs on the solver's stream.  Returns
    (problem, cost history)."""
    import torch
    pipe = DevicePipeline(prob, solver, param="se3", loss=loss)
    dev, n = pipe.res.device, solver.order()
    H = torch.empty(solver.dataSize(), dtype=torch.float64, device=dev)
    g = torch.empty(n, dtype=torch.float64, device=dev)
    step = torch.empty_like(g)
    trip = torch.empty(3, dtype=torch.float64, device=dev)   # cost, new_cost, 0.5 g.step
    hist = []
    last_failed = last_ok = last_good = 0
    with torch.cuda.stream(solver._torch_stream(dev)):
        for i in range(max_iters):
            pipe.linearize()
            pipe.apply_loss()
            pipe.cost_linearized(out=trip[0:1])
            H.zero_()
            g.zero_()
            if ordered_fill:
                pipe.fill_hessian_ordered(H, g, lam)
            else:
                pipe.fill_hessian(H, g, lam)
            step.copy_(g)
            solver.factor(H)
            solver.solve(H, step, n, 1)
            cams, pts = pipe.apply_step(step)
            pipe.cost(cams, pts, out=trip[1:2])
            torch.dot(g, step, out=trip[2])
            trip[2].mul_(0.5)
            cost, new_cost, model_red = trip.tolist()   # the iteration's only device-to-host read
            bad, good = new_cost > cost, new_cost < cost * 0.999
            hist.append((cost, new_cost, lam))
            if log:
                log("[%d] cost %.3e -> %.3e lambda %.1e" % (i, cost, new_cost, lam))
            if bad:
                last_failed = i
                if lam > 1e8 or i > last_ok + 15:
                    break
                lam *= 3
                continue
            pipe.set_params(cams, pts)
            last_ok = i
            if good:
                last_good = i
            rel_red = (cost - new_cost) / model_red if model_red != 0 else 0.0
            if rel_red > 0.6:
                lam *= 0.6
            elif rel_red < 0.4:
                lam *= 1.3
            if i >= last_good + 3 and i >= last_failed + 3:
                break
    return pipe.to_problem(), hist


LOSS_KINDS = {"huber": 1, "cauchy": 2}   # bsp_bal_loss_f64's kind; 0 = trivial (loss=None)

_I64P = ctypes.POINTER(ctypes.c_int64)


class BalFillPlan:
    """the host plan of the ordered Hessian fill (bsp_bal_fill_plan_create, csrc/bal_fill_plan.h): the
    observations grouped by point and by camera, the (point, camera) pairs with their blocks, and the camera
    lists cut into chunks.  obs_cam / obs_pt are host arrays; observations with an index out of range are
    left out.  Built without a GPU; keeps its solver alive."""

    INFO_KEYS = ("kept", "skipped", "pairs", "chunks", "C", "W", "max_pt_list", "max_cam_list", "scratch_len",
                 "host_bytes", "device_bytes", "cam_size")

    def __init__(self, solver, cam_size, num_pts, num_cams, obs_cam, obs_pt, num_obs=None):
        from . import _check
        self._lib = _lib.load()
        self._h = None
        oc = np.ascontiguousarray(obs_cam, dtype=np.int64)
        op = np.ascontiguousarray(obs_pt, dtype=np.int64)
        if oc.ndim != 1 or oc.shape != op.shape:
            raise ValueError("BalFillPlan: obs_cam and obs_pt must be one-dimensional and of one length")
        n = len(oc) if num_obs is None else int(num_obs)
        h = ctypes.c_void_p()
        _check(self._lib.bsp_bal_fill_plan_create(
            solver._h, ctypes.c_int32(cam_size), ctypes.c_int64(num_pts), ctypes.c_int64(num_cams),
            ctypes.c_int64(n), oc.ctypes.data_as(_I64P), op.ctypes.data_as(_I64P), ctypes.byref(h)))
        self._h = h
        self.solver, self.cam_size, self.num_obs = solver, int(cam_size), n

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.bsp_bal_fill_plan_destroy(h)

    def info(self):
        """figures of the plan (bsp_bal_fill_plan_info): kept / skipped observations, pairs, chunks, the
        chunk length C and lanes per element W of the build, the longest point and camera list, the scratch
        length in doubles, and its bytes on the host and on the device"""
        from . import _check
        out = (ctypes.c_int64 * 12)()
        _check(self._lib.bsp_bal_fill_plan_info(self._h, out))
        return dict(zip(self.INFO_KEYS, [int(x) for x in out]))

    def _testTables(self):
        """TESTING: every table of the plan as int64 arrays (bsp_test_bal_fill_plan)"""
        from . import _check
        need = ctypes.c_int64(0)
        _check(self._lib.bsp_test_bal_fill_plan(self._h, None, ctypes.c_int64(0), ctypes.byref(need)))
        buf = np.empty(need.value, dtype=np.int64)
        _check(self._lib.bsp_test_bal_fill_plan(self._h, buf.ctypes.data_as(_I64P), need, ctypes.byref(need)))
        keys = ("numPts", "numCams", "camSize", "kept", "skipped", "nPairs", "nChunks", "C", "W", "scratchLen")
        out = dict(zip(keys, (int(x) for x in buf[:10])))
        npt, nc, kept, nq, nk = out["numPts"], out["numCams"], out["kept"], out["nPairs"], out["nChunks"]
        pos = 10
        for name, rows in (("ptPtr", npt + 1), ("ptObs", kept), ("pairPtr", nq + 1), ("pairCam", nq),
                           ("pairPt", nq), ("pairOff", nq), ("pairStride", nq), ("pairFlip", nq),
                           ("camPtr", nc + 1), ("camObs", kept), ("camChunkPtr", nc + 1), ("chunkCam", nk),
                           ("chunkBegin", nk), ("chunkEnd", nk), ("ptDiagOff", npt), ("ptDiagStride", npt),
                           ("ptStart", npt), ("camDiagOff", nc), ("camDiagStride", nc), ("camStart", nc)):
            out[name] = buf[pos:pos + rows].copy()
            pos += rows
        assert pos == len(buf)
        return out


class DevicePipeline:
    """problem data resident on the GPU + the two device stages of a Gauss-Newton / LM iteration.
    param = "bal9": cameras are the 9 parameters of a BAL file (BAL_bench's block size, derivatives
    by dual numbers); param = "se3": the reference optimizer's parameterisation (6-wide SE3-tangent
    camera blocks, calibration fixed, closed-form Jacobians of BaAtLarge.h:56-150).
    loss = None, ("huber", a) or ("cauchy", a): the robust loss apply_loss() and cost() use
    (examples/SoftLoss.h); None leaves every other method as it is without one."""

    def __init__(self, prob, solver, device="cuda", param="bal9", loss=None):
        import torch
        assert param in ("bal9", "se3")
        if loss is None:
            self.loss_kind, self.loss_a = 0, 1.0
        else:
            name, a = loss
            if name not in LOSS_KINDS:
                raise ValueError("loss must be None, ('huber', a) or ('cauchy', a), got %r" % (loss,))
            self.loss_kind, self.loss_a = LOSS_KINDS[name], float(a)
        self.rho = self._cand_res = self._cand_rho = self._sum_scratch = self._fill_plan = None
        self.param = param
        self.cam_size = 9 if param == "bal9" else 6
        self.prob, self.solver = prob, solver
        self.lib = _lib.load()
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.obs_cam, self.obs_pt = t(prob.obs_cam, np.int64), t(prob.obs_pt, np.int64)
        self.obs_xy = t(prob.obs_xy, np.float64)
        self.cams, self.pts = t(prob.cams, np.float64), t(prob.pts, np.float64)
        n = len(prob.obs_cam)
        self.res = torch.empty(2 * n, dtype=torch.float64, device=device)
        self.Jc = torch.empty(2 * self.cam_size * n, dtype=torch.float64, device=device)
        self.Jp = torch.empty(6 * n, dtype=torch.float64, device=device)
        self.n_obs = n

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(0 if t is None else t.data_ptr())

    def _stream(self, stream):
        """the stream of a launch: `stream` if given (torch.cuda.Stream or raw hipStream_t address), else
        what the solver's setStream() was last given, looked up at call time; None = the default stream"""
        s = self.solver._stream if stream is None else stream
        return ctypes.c_void_p(0 if s is None else getattr(s, "cuda_stream", s))

    def linearize(self, stream=None):
        """residuals and Jacobians of every observation (bsp_bal_linearize_f64), on the solver's stream
        or on `stream`"""
        from . import _check
        fn = self.lib.bsp_bal_linearize_f64 if self.param == "bal9" else self.lib.bsp_bal_linearize_se3_f64
        _check(fn(
            ctypes.c_int64(self.n_obs), self._p(self.obs_cam), self._p(self.obs_pt), self._p(self.obs_xy),
            self._p(self.cams), self._p(self.pts), self._p(self.res), self._p(self.Jc), self._p(self.Jp),
            self._stream(stream)))
        return self.res

    def fill_hessian(self, data, grad=None, lam=0.0, dbg=None, stream=None):
        """data (zeroed by the caller) += J^T J through the device accessor, grad += J^T r,
        LM damping (bsp_bal_fill_hessian_*), on the solver's stream or on `stream`"""
        import torch
        from . import _check
        f32 = data.dtype == torch.float32
        lam_c = ctypes.c_float(lam) if f32 else ctypes.c_double(lam)
        head = (self.solver._h, ctypes.c_int64(self.prob.num_pts), ctypes.c_int64(self.prob.num_cams),
                ctypes.c_int64(self.n_obs), self._p(self.obs_cam), self._p(self.obs_pt), self._p(self.Jc),
                self._p(self.Jp), self._p(self.res), lam_c, self._p(data), self._p(grad))
        if self.param == "se3":
            fn = self.lib.bsp_bal_fill_hessian_se3_f32 if f32 else self.lib.bsp_bal_fill_hessian_se3_f64
            _check(fn(*head, self._stream(stream)))
        else:
            fn = self.lib.bsp_bal_fill_hessian_f32 if f32 else self.lib.bsp_bal_fill_hessian_f64
            _check(fn(*head, self._p(dbg), self._stream(stream)))
        return data

    def fill_plan(self):
        """the BalFillPlan of prob's observation list for this solver, built on first use and kept"""
        if self._fill_plan is None:
            self._fill_plan = BalFillPlan(self.solver, self.cam_size, self.prob.num_pts, self.prob.num_cams,
                                          self.prob.obs_cam, self.prob.obs_pt)
        return self._fill_plan

    def fill_hessian_ordered(self, data, grad=None, lam=0.0, stream=None):
        """fill_hessian without atomics (bsp_bal_fill_ordered_*): the same contract, with every sum taken in
        the order the plan fixes, so that data and grad are the same bits on every run.  The plan is built
        on the host from prob's observation list on first use (fill_plan()); Jc / Jp / res must hold those
        observations.  On the solver's stream or on `stream`."""
        import torch
        from . import _check
        plan = self.fill_plan()
        if plan.num_obs != self.n_obs:
            raise ValueError("fill_hessian_ordered: the plan holds %d observations, the pipeline %d"
                             % (plan.num_obs, self.n_obs))
        f32 = data.dtype == torch.float32
        fn = self.lib.bsp_bal_fill_ordered_f32 if f32 else self.lib.bsp_bal_fill_ordered_f64
        _check(fn(self.solver._h, plan._h, self._p(self.Jc), self._p(self.Jp), self._p(self.res),
                  ctypes.c_float(lam) if f32 else ctypes.c_double(lam), self._p(data), self._p(grad),
                  self._stream(stream)))
        return data

    # ---- the rest of an LM iteration (bsp_bal_residuals / loss / sum / apply_step); like the two stages
    # above, every launch goes to the stream _stream() resolves and nothing synchronises the host
    def _empty(self, n):
        import torch
        return torch.empty(n, dtype=torch.float64, device=self.res.device)

    def residuals(self, cams=None, pts=None, out=None, stream=None):
        """the residuals alone (2 per observation) at `cams` / `pts`, the pipeline's own by default, into
        `out` (a new tensor by default): what linearize() leaves in res, without the Jacobians"""
        from . import _check
        out = self._empty(2 * self.n_obs) if out is None else out
        fn = self.lib.bsp_bal_residuals_f64 if self.param == "bal9" else self.lib.bsp_bal_residuals_se3_f64
        _check(fn(
            ctypes.c_int64(self.n_obs), self._p(self.obs_cam), self._p(self.obs_pt), self._p(self.obs_xy),
            self._p(self.cams if cams is None else cams), self._p(self.pts if pts is None else pts),
            self._p(out), self._stream(stream)))
        return out

    def _loss(self, res, Jc, Jp, rho, stream):
        from . import _check
        _check(self.lib.bsp_bal_loss_f64(
            ctypes.c_int64(self.n_obs), ctypes.c_int32(self.cam_size), ctypes.c_int32(self.loss_kind),
            ctypes.c_double(self.loss_a), self._p(res), self._p(Jc), self._p(Jp), self._p(rho),
            self._stream(stream)))
        return rho

    def _sum(self, x, scale, out, stream):
        import torch
        from . import _check
        n = x.numel()
        need = int(self.lib.bsp_bal_sum_scratch_len(ctypes.c_int64(n)))
        if self._sum_scratch is None or self._sum_scratch.numel() < need:
            self._sum_scratch = self._empty(need)
        out = torch.empty((), dtype=torch.float64, device=x.device) if out is None else out
        _check(self.lib.bsp_bal_sum_f64(ctypes.c_int64(n), self._p(x), ctypes.c_double(scale),
                                        self._p(self._sum_scratch), self._p(out), self._stream(stream)))
        return out.reshape(())

    def apply_loss(self, stream=None):
        """after linearize(): rho (one per observation) of the squared residuals into self.rho and, for a
        robust loss, res / Jc / Jp scaled in place by sqrt(rho') so that fill_hessian accumulates
        rho' J^T J and rho' J^T r (observations with rho' == 1 are not rewritten)"""
        if self.rho is None or self.rho.numel() != self.n_obs:
            self.rho = self._empty(self.n_obs)
        return self._loss(self.res, self.Jc, self.Jp, self.rho, stream)

    def cost_linearized(self, out=None, stream=None):
        """0.5 * sum of self.rho (apply_loss), a 0-dim device tensor (or `out`, one element)"""
        return self._sum(self.rho, 0.5, out, stream)

    def cost(self, cams=None, pts=None, out=None, stream=None):
        """0.5 * sum rho(|r|^2) at `cams` / `pts` (the pipeline's own by default) from the residual-only
        kernel (computeCost, BaAtLargeOptimizer.cpp:54-63, with the loss): a 0-dim device tensor (or
        `out`, one element).  res / Jc / Jp / rho of the linearisation are left alone."""
        if self._cand_res is None or self._cand_res.numel() != 2 * self.n_obs:
            self._cand_res, self._cand_rho = self._empty(2 * self.n_obs), self._empty(self.n_obs)
        self.residuals(cams, pts, out=self._cand_res, stream=stream)
        self._loss(self._cand_res, None, None, self._cand_rho, stream)
        return self._sum(self._cand_rho, 0.5, out, stream)

    def apply_step(self, step, stream=None):
        """applyStep (BaAtLargeOptimizer.cpp:173-184) of `step` (the solver's internal order: what
        solve() leaves in the gradient buffer) as NEW tensors (cams, pts); the pipeline's own parameters
        stay, so rejecting the step costs nothing.  bal9: parameters minus step; se3: points minus step,
        T_W_C <- exp(-step) T_W_C (rotation vector of length <= pi), calibration copied.  (With a side
        stream on the solver, call under torch.cuda.stream(...) of that stream, as for any tensor that is
        allocated here and used there.)"""
        import torch
        from . import _check
        cams, pts = torch.empty_like(self.cams), torch.empty_like(self.pts)
        fn = self.lib.bsp_bal_apply_step_f64 if self.param == "bal9" else self.lib.bsp_bal_apply_step_se3_f64
        _check(fn(self.solver._h, ctypes.c_int64(self.prob.num_pts), ctypes.c_int64(self.prob.num_cams),
                  self._p(self.cams), self._p(self.pts), self._p(step), self._p(cams), self._p(pts),
                  self._stream(stream)))
        return cams, pts

    def set_params(self, cams, pts):
        """make (cams, pts) -- device tensors, e.g. what apply_step returned -- the pipeline's parameters"""
        assert cams.numel() == self.cams.numel() and pts.numel() == self.pts.numel()
        self.cams, self.pts = cams, pts

    def to_problem(self):
        """the pipeline's parameters downloaded into a BalProblem (waits for the solver's stream)"""
        self.solver._torch_stream(self.cams.device).synchronize()
        return BalProblem(self.cams.cpu().numpy(), self.pts.cpu().numpy(), self.prob.obs_cam, self.prob.obs_pt,
                          self.prob.obs_xy)
