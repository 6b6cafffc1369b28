"""An independent reference for the device LM step of the BAL pipeline (csrc/bal_pipeline.hip: robust loss,
fixed-order sum, retraction; baspacho_amd/bal.py: lm_optimize_device).

Nothing here shares a formula with the kernels:

* mpmath at 70 digits: rho and rho' of the three losses (examples/SoftLoss.h); the SE3 retraction
  T <- exp(-step) T from ROTATION MATRICES, R' = exp(-[w]x) R(w_cam), t' = exp(-[w]x) t + V(-w)(-u), with the
  closed forms of Rodrigues and V (the kernels compose quaternions and use series); the cost of a problem
  from bal_ref.residual_se3;
* a float64 host model of each piece -- the YARDSTICK, not the code under test: quaternion composition, series
  for b and c, np.log1p.  tests/test_bal_step_cpu.py measures it against mpmath; the bounds the kernels are
  held to are 8 x its worst errors (fma contraction, the device's sin / cos / atan2 / log1p), as for
  bal_ref.LIN_BOUND;
* the numpy restatement of balSum's summation order;
* a Levenberg-Marquardt loop on dense normal equations with the loss weights (lm_host), the schedule of
  bal.lm_optimize, for the end-to-end conditions.

Only tests/ may import this file.  Nothing here touches the GPU."""
import numpy as np

import bal_ref as R

DPS = R.DPS
EPS = float(np.finfo(np.float64).eps)
KINDS = {"trivial": 0, "huber": 1, "cauchy": 2}

# The float64 host models against mpmath (tests/test_bal_step_cpu.py measures and prints them):
#   retraction over STEP_CASES: max |R(w_out) - R_ref| and |t_out - t_ref| / (|t| + |u|)
#   loss over loss_cases(): relative error of rho, sqrt(w) and the scaled words
STEP_WORST_R_MEASURED = 3.4e-16   # "lands 1e-3 past pi"; 1e-17 .. 1.5e-16 on the generic cases
STEP_WORST_T_MEASURED = 1.6e-16   # "step rotation 3.0"
LOSS_WORST_MEASURED = 2.3e-16     # a Cauchy-scaled word; rho of Huber 2.2e-16
STEP_BOUND_R = 8 * STEP_WORST_R_MEASURED
STEP_BOUND_T = 8 * STEP_WORST_T_MEASURED
LOSS_BOUND = 8 * LOSS_WORST_MEASURED
assert STEP_BOUND_R <= 1e-13 and STEP_BOUND_T <= 1e-13 and LOSS_BOUND <= 64 * EPS


def _mp():
    import mpmath
    return mpmath


def _f(v):
    return _mp().mpf(float(v))


# ---- losses (mpmath) -----------------------------------------------------------------------------------
def rho_mp(kind, a, s):
    """rho(s) of the loss `kind` (name or number) with size a; s, a mpf"""
    mp = _mp()
    kind = KINDS.get(kind, kind)
    if kind == 0:
        return s
    if kind == 1:
        return 2 * a * mp.sqrt(s) - a * a if s > a * a else s
    return a * a * mp.log(1 + s / (a * a))


def drho_mp(kind, a, s):
    """rho'(s)"""
    mp = _mp()
    kind = KINDS.get(kind, kind)
    if kind == 0:
        return mp.mpf(1)
    if kind == 1:
        return a / mp.sqrt(s) if s > a * a else mp.mpf(1)
    return 1 / (1 + s / (a * a))


def loss_reference(kind, a, res):
    """per observation (rho, sqrt(w)) as mpf lists, s = r0^2 + r1^2 exactly from the float64 residuals"""
    mp = _mp()
    with mp.workdps(DPS):
        am = _f(a)
        out_r, out_q = [], []
        for r0, r1 in np.asarray(res, dtype=np.float64).reshape(-1, 2):
            s = _f(r0) * _f(r0) + _f(r1) * _f(r1)
            out_r.append(rho_mp(kind, am, s))
            out_q.append(mp.sqrt(drho_mp(kind, am, s)))
        return out_r, out_q


def _rel(got, want):
    """relative error of a float against an mpf; an exact zero must be met exactly"""
    mp = _mp()
    if want == 0:
        return 0.0 if got == 0 else float("inf")
    if not np.isfinite(got):
        return float("inf")
    return float(abs(_f(got) - want) / abs(want))


def loss_errors(kind, a, res, rho, scaled):
    """worst relative error of rho (n) and of the scaled words against mpmath; `scaled` is a list of
    (before, after) array pairs, each (n, k): after = before * sqrt(w) of its observation.  Returns
    (rho error, word error)."""
    mp = _mp()
    rr, qq = loss_reference(kind, a, res)
    with mp.workdps(DPS):
        e_rho = max([_rel(g, w) for g, w in zip(np.asarray(rho).ravel(), rr)] or [0.0])
        e_w = 0.0
        for before, after in scaled:
            b, t = np.asarray(before).reshape(len(rr), -1), np.asarray(after).reshape(len(rr), -1)
            for o in range(len(rr)):
                for x, y in zip(b[o], t[o]):
                    e_w = max(e_w, _rel(y, _f(x) * qq[o]))
        return e_rho, e_w


def unit_weight(kind, a, res):
    """which observations have w == 1 by the loss's definition (their words must stay bitwise intact):
    the trivial loss, Huber with s <= a^2, any s == 0"""
    kind = KINDS.get(kind, kind)
    res = np.asarray(res, dtype=np.float64).reshape(-1, 2)
    mp = _mp()
    with mp.workdps(DPS):
        s = [_f(r0) * _f(r0) + _f(r1) * _f(r1) for r0, r1 in res]
        if kind == 0:
            return np.ones(len(res), dtype=bool)
        if kind == 1:
            return np.array([v <= _f(a) * _f(a) for v in s], dtype=bool)
        return np.array([v == 0 for v in s], dtype=bool)


def loss_cases(a, n, seed=0):
    """(n, 2) residuals that cycle through the edges of the losses of size a (a exactly representable, e.g.
    2): s = 0, below a^2, exactly a^2, one ulp above a^2, far above, the behind-the-camera row (25, 0), and
    random ones of both kinds.  Returns (res, is_fixed_row)."""
    rng = np.random.default_rng(seed)
    one_ulp = float(np.sqrt(np.spacing(a * a)))       # a^2 + one_ulp^2 = the float after a^2, exactly
    assert a * a + one_ulp * one_ulp == np.nextafter(a * a, np.inf)
    edges = [(0.0, 0.0), (0.3 * a, -0.4 * a), (a, 0.0), (a, one_ulp), (-30.0 * a, 17.0 * a), (25.0, 0.0),
             (0.0, -a), (1e-9 * a, 0.0)]
    res = np.empty((n, 2))
    for o in range(n):
        k = o % (len(edges) + 2)
        if k < len(edges):
            res[o] = edges[k]
        else:
            res[o] = rng.standard_normal(2) * (0.4 * a if k == len(edges) else 6.0 * a)
    fixed = np.array([tuple(r) == (25.0, 0.0) for r in res])
    return res, fixed


# ---- losses (float64 host model) ---------------------------------------------------------------------
def loss_model(kind, a, res):
    """(rho (n), sqrt(w) (n)) in float64 numpy: the yardstick"""
    kind = KINDS.get(kind, kind)
    res = np.asarray(res, dtype=np.float64).reshape(-1, 2)
    s = res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]
    if kind == 0:
        return s.copy(), np.ones_like(s)
    a2 = a * a
    if kind == 1:
        out = s > a2
        r = np.sqrt(np.where(out, s, 1.0))
        return np.where(out, 2.0 * a * r - a2, s), np.where(out, np.sqrt(a / r), 1.0)
    x = s / a2
    return a2 * np.log1p(x), np.sqrt(1.0 / (1.0 + x))


# ---- retraction (mpmath, rotation matrices) ----------------------------------------------------------
def _skew_mp(w):
    mp = _mp()
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def rotation_mp(w):
    """exp([w]x) by Rodrigues' closed form at the working precision"""
    mp = _mp()
    th = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th == 0:
        return mp.eye(3)
    K = _skew_mp(w)
    return mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)


def retract_se3_mp(cam, step):
    """(R', t') of T <- exp(-step) T for cam = [w(3), t(3), ..] and step = (u, w): mp matrices"""
    mp = _mp()
    w_cam, t = [_f(v) for v in cam[0:3]], mp.matrix([_f(v) for v in cam[3:6]])
    u, d = mp.matrix([-_f(v) for v in step[0:3]]), [-_f(v) for v in step[3:6]]
    Rd = rotation_mp(d)
    th = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if th == 0:
        V = mp.eye(3)
    else:
        K = _skew_mp(d)
        V = mp.eye(3) + ((1 - mp.cos(th)) / th ** 2) * K + ((th - mp.sin(th)) / th ** 3) * (K * K)
    return Rd * rotation_mp(w_cam), Rd * t + V * u


def step_errors(cams, steps, cams_out):
    """per case: (max |R(w_out) - R_ref|, |t_out - t_ref|_2 / (|t|_2 + |u|_2)) of retracted cameras
    (n, 9) against the mpmath retraction, R(w_out) evaluated in mpmath from the float64 output"""
    mp = _mp()
    eR, eT = [], []
    with mp.workdps(DPS):
        for cam, stp, out in zip(cams, steps, cams_out):
            Rr, tr = retract_se3_mp(cam, stp)
            Ro = rotation_mp([_f(v) for v in out[0:3]])
            eR.append(float(max(abs(Ro[i, j] - Rr[i, j]) for i in range(3) for j in range(3))))
            dt = mp.sqrt(sum((_f(out[3 + i]) - tr[i]) ** 2 for i in range(3)))
            scale = mp.sqrt(sum(_f(v) ** 2 for v in cam[3:6])) + mp.sqrt(sum(_f(v) ** 2 for v in stp[0:3]))
            eT.append(float(dt / scale) if scale != 0 else (0.0 if dt == 0 else float("inf")))
    return np.array(eR), np.array(eT)


def _step_cases():
    """(names, cams (n, 9), steps (n, 6)): camera (w, t) and step (u, w) of every case"""
    rng = np.random.default_rng(17)
    calib = lambda: [800.0 + rng.uniform(-20, 20), 1e-2 * rng.standard_normal(), 1e-4 * rng.standard_normal()]
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.standard_normal(3))
    names, cams, steps = [], [], []

    def add(name, w_cam, w_step, u=None, t=None):
        names.append(name)
        cams.append(np.concatenate([w_cam, 3.0 * rng.standard_normal(3) if t is None else t, calib()]))
        steps.append(np.concatenate([rng.standard_normal(3) if u is None else u, w_step]))
    for k in range(20):
        add("generic%d" % k, 0.6 * unit() * rng.uniform(0.5, 1.5), 1e-2 * rng.standard_normal(3),
            u=0.1 * rng.standard_normal(3))
    add("zero step", 0.6 * unit(), np.zeros(3), u=np.zeros(3))
    add("step rotation 1e-9", 0.6 * unit(), 1e-9 * unit())
    add("step rotation 1e-160", 0.6 * unit(), 1e-160 * unit())
    add("camera rotation 0", np.zeros(3), 1e-2 * rng.standard_normal(3))
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    for name, total in (("lands at pi - 1e-9", np.pi - 1e-9), ("lands at pi", np.pi), ("lands 1e-3 past pi", np.pi + 1e-3)):
        add(name, 2.0 * axis, -(total - 2.0) * axis)     # exp(-w) turns by |w| about the camera's own axis
    add("step rotation 3.0", 0.6 * unit(), 3.0 * unit())
    w = 0.7 * unit()
    add("step undoes the camera rotation to 1e-12", w, w - 1e-12 * unit())
    return names, np.array(cams), np.array(steps)


STEP_NAMES, STEP_CAMS, STEP_STEPS = _step_cases()
STEP_CASES = list(zip(STEP_NAMES, STEP_CAMS, STEP_STEPS))
for _a in (STEP_CAMS, STEP_STEPS):
    _a.setflags(write=False)
assert (STEP_STEPS[STEP_NAMES.index("step rotation 1e-160"), 3:] ** 2).sum() < np.finfo(np.float64).tiny, \
    "theta^2 must underflow (to a subnormal)"


# ---- retraction (float64 host model) -------------------------------------------------------------------
def _series(x, first, terms):
    """sum_k (-x)^k / (first + 2k)!, Horner, float64"""
    from math import factorial
    c = [1.0 / factorial(first + 2 * k) for k in range(terms)]
    out = np.full_like(x, c[-1])
    for k in range(terms - 2, -1, -1):
        out = out * (-x) + c[k]
    return out


def _abc(x):
    """a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3 as functions of x = th^2: series
    below x = 0.25, closed forms above (b by the half angle)"""
    small = x < 0.25
    th = np.sqrt(np.where(small, 1.0, x))
    xs = np.where(small, 1.0, x)
    sh = np.sin(0.5 * th)
    xl = np.where(small, x, 0.0)
    return (np.where(small, _series(xl, 1, 9), np.sin(th) / th), np.where(small, _series(xl, 2, 9), 2 * sh * sh / xs),
            np.where(small, _series(xl, 3, 9), (th - np.sin(th)) / (th * xs)))


def _quat(v):
    """unit quaternions (n, 4), scalar first, of axis-angle vectors (n, 3)"""
    x = np.sum(v * v, axis=1)
    small = x < 1e-4
    th = np.sqrt(np.where(small, 1.0, x))
    k = np.where(small, 0.5 - x / 48.0 + x * x / 3840.0, np.sin(0.5 * th) / th)
    q0 = np.where(small, 1.0 - x / 8.0 + x * x / 384.0 - x ** 3 / 46080.0, np.cos(0.5 * th))
    return np.concatenate([q0[:, None], k[:, None] * v], axis=1)


def retract_se3_model(cams, steps):
    """T <- exp(-step) T on arrays in float64: cameras (n, 9), steps (n, 6) = (u, w) -> cameras (n, 9)"""
    cams, steps = np.asarray(cams, dtype=np.float64), np.asarray(steps, dtype=np.float64)
    out = cams.copy()
    d, u, t = -steps[:, 3:6], -steps[:, 0:3], cams[:, 3:6]
    a, b, c = (v[:, None] for v in _abc(np.sum(d * d, axis=1)))
    dt, du = np.cross(d, t), np.cross(d, u)
    out[:, 3:6] = (t + a * dt + b * np.cross(d, dt)) + (u + b * du + c * np.cross(d, du))
    p, r = _quat(d), _quat(cams[:, 0:3])
    q = np.concatenate([(p[:, 0] * r[:, 0] - np.sum(p[:, 1:] * r[:, 1:], axis=1))[:, None],
                        p[:, 0:1] * r[:, 1:] + r[:, 0:1] * p[:, 1:] + np.cross(p[:, 1:], r[:, 1:])], axis=1)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q = np.where(q[:, 0:1] < 0, -q, q)
    n = np.linalg.norm(q[:, 1:], axis=1)
    small = n < 1e-4
    ns = np.where(small, 1.0, n)
    q0s = np.where(small, q[:, 0], 1.0)
    z2 = (np.where(small, n, 0.0) / q0s) ** 2
    k = np.where(small, 2.0 / q0s * (1.0 - z2 / 3.0 + z2 * z2 / 5.0), 2.0 * np.arctan2(ns, q[:, 0]) / ns)
    out[:, 0:3] = k[:, None] * q[:, 1:]
    return out


# ---- the summation order of balSum ---------------------------------------------------------------------
SUM_CHUNK, SUM_WIDTH = 2048, 256


def _fold(acc):
    """rows of SUM_WIDTH thread sums -> entry 0 after the LDS fold s = 128, 64, .. 1"""
    acc = acc.copy()
    s = SUM_WIDTH // 2
    while s > 0:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    return acc[:, 0]


def _strided_sum(x):
    """x padded with +0.0 to rows of SUM_WIDTH: thread t adds x[t], x[t + 256], .. from +0.0, then the fold
    (adding +0.0 to a sum that started at +0.0 never changes a bit)"""
    rows = -(-len(x) // SUM_WIDTH)
    xp = np.zeros(rows * SUM_WIDTH)
    xp[:len(x)] = x
    acc = np.zeros(SUM_WIDTH)
    for row in xp.reshape(rows, SUM_WIDTH):
        acc = acc + row
    return _fold(acc[None, :])[0]


def sum_model(x, scale):
    """bitwise what bsp_bal_sum_f64 writes to out[0]"""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return np.float64(0.0)
    nparts = -(-len(x) // SUM_CHUNK)
    xp = np.zeros(nparts * SUM_CHUNK)
    xp[:len(x)] = x
    A = xp.reshape(nparts, SUM_CHUNK // SUM_WIDTH, SUM_WIDTH)
    acc = np.zeros((nparts, SUM_WIDTH))
    for m in range(A.shape[1]):
        acc = acc + A[:, m, :]
    return np.float64(scale) * _strided_sum(_fold(acc))


# ---- cost of a problem (mpmath) and the host LM ------------------------------------------------------
def cost_mp(prob, kind=0, a=1.0):
    """0.5 sum rho(|r|^2) over the observations, SE3 residual with the behind-the-camera rule; returns
    (cost as float, per-observation (|r0| + |r1|, rho) as floats for error bounds)"""
    mp = _mp()
    with mp.workdps(DPS):
        zero6, zero3, am = [mp.mpf(0)] * 6, [mp.mpf(0)] * 3, _f(a)
        total, terms = mp.mpf(0), []
        for c, p, xy in zip(prob.obs_cam, prob.obs_pt, prob.obs_xy):
            r = R.residual_se3([_f(v) for v in prob.cams[c]], [_f(v) for v in prob.pts[p]], [_f(v) for v in xy],
                               zero6, zero3)
            rho = rho_mp(kind, am, r[0] * r[0] + r[1] * r[1])
            total += rho
            terms.append((float(abs(r[0]) + abs(r[1])), float(rho)))
        return float(total / 2), np.array(terms)


def outlier_scene(seed=3):
    """synth_scene(14, 300, seed, perturb=2e-2) with 5 % of the observations corrupted: each coordinate
    shifted by +/- uniform(40, 80) px.  Returns (problem, inlier mask)."""
    from baspacho_amd import bal
    prob = bal.synth_scene(14, 300, seed=seed, perturb=2e-2)
    nobs = len(prob.obs_cam)
    rng = np.random.default_rng(100 + seed)
    bad = rng.choice(nobs, nobs // 20, replace=False)
    xy = prob.obs_xy.copy()
    xy[bad] += rng.choice([-1.0, 1.0], (len(bad), 2)) * rng.uniform(40, 80, (len(bad), 2))
    inlier = np.ones(nobs, dtype=bool)
    inlier[bad] = False
    return bal.BalProblem(prob.cams, prob.pts, prob.obs_cam, prob.obs_pt, xy), inlier


def inlier_cost(prob, inlier):
    """0.5 sum |r|^2 over the uncorrupted observations, on the host"""
    from oracle import bal_model
    res, _, _ = bal_model.linearize_se3(prob.cams[prob.obs_cam], prob.pts[prob.obs_pt], prob.obs_xy)
    return 0.5 * float(np.sum(res[inlier] ** 2))


def noise_floor(n_obs):
    """0.5 px of Gaussian noise on 2 coordinates per observation"""
    return 0.5 * 0.25 * 2 * n_obs


def lm_host(prob, loss=None, max_iters=50, lam=1e-5):
    """bal.lm_optimize's loop on the host with DENSE normal equations in the caller's parameter order
    (points first), the loss weights applied as H = J^T W J, g = J^T W r, cost = 0.5 sum rho, and the float64
    retraction model.  loss: None, ("huber", a) or ("cauchy", a).  Returns (problem, history)."""
    from baspacho_amd import bal
    from oracle import bal_model
    kind, a = (0, 1.0) if loss is None else (KINDS[loss[0]], float(loss[1]))
    npt, nc = prob.num_pts, prob.num_cams

    def cost_of(p):
        res, _, _ = bal_model.linearize_se3(p.cams[p.obs_cam], p.pts[p.obs_pt], p.obs_xy)
        return 0.5 * float(loss_model(kind, a, res)[0].sum())
    hist = []
    last_failed = last_ok = last_good = 0
    for i in range(max_iters):
        res, Jc, Jp = bal_model.linearize_se3(prob.cams[prob.obs_cam], prob.pts[prob.obs_pt], prob.obs_xy)
        rho, sq = loss_model(kind, a, res)
        cost = 0.5 * float(rho.sum())
        J = R.dense_jacobian(npt, nc, 6, prob.obs_cam, prob.obs_pt, Jc, Jp) * np.repeat(sq, 2)[:, None]
        r = (res * sq[:, None]).ravel()
        H, g = J.T @ J, J.T @ r
        idx = np.arange(len(g))
        H[idx, idx] = H[idx, idx] * (1 + lam) + lam * 1e-3
        step = np.linalg.solve(H, g)
        cand = bal.BalProblem(retract_se3_model(prob.cams, step[3 * npt:].reshape(nc, 6)),
                              prob.pts - step[:3 * npt].reshape(npt, 3), prob.obs_cam, prob.obs_pt, prob.obs_xy)
        model_red = 0.5 * float(g @ step)
        new_cost = cost_of(cand)
        bad, good = new_cost > cost, new_cost < cost * 0.999
        hist.append((cost, new_cost, lam))
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
