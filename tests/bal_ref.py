"""An independent reference for the BAL caller pipeline (csrc/bal_pipeline.hip, baspacho_amd/bal.py).

Nothing here shares a formula, an accessor or a rounding with the code under test:

* the residual of one observation in mpmath at 70 digits, for the 9-parameter BAL camera and for the SE3
  parameterisation (T <- exp(delta) T, translation first, with the behind-the-camera rule).  The rotation
  goes through a unit quaternion, which neither kernel does; at theta = 0 it is the identity;
* the Jacobians are central differences of those residual functions (step 1e-25: truncation ~ h^2 f''' / 6
  ~ 1e-45, rounding ~ 1e-70 / h ~ 1e-45, both far below 1e-25).  There is no derivative formula in this
  file; tests/test_bal_ref_cpu.py checks two steps a factor of 10 apart against each other;
* the normal equations are built densely from J in the caller's parameter order, in np.longdouble, with
  the sum of the absolute products and the number of terms per element, and reach the solver's layout
  through the skeleton (element_coords) and scalarPermutation() alone -- no host accessor on that path.

Only tests/ may import this file.  Nothing here touches the GPU."""
import numpy as np

DPS = 70
STEP_EXP = -25

# theta^2 cuts of the code under test: reproject() switches from the closed forms to the series at
# BAL9_CUT, rodriguesMatrix() to its constants at SE3_CUT (the linearisation cases straddle both)
BAL9_CUT = 0.25
SE3_CUT = 1e-20

# The float64 host model (oracle/bal_model.py) against this reference, worst scaled error over LIN_CASES and
# both parameterisations (tests/test_bal_ref_cpu.py measures and prints it): 1.03e-14, a bal9 Jacobian entry
# of the case "special"; residuals 3.1e-16.  The kernels are held to 8 x that (fma contraction, the device's
# sin / cos).  The bound must stay below 1e-12: the k = w / theta defect sits at 1e-9 .. 4e-8.
LIN_WORST_MEASURED = 1.03e-14
LIN_BOUND = 8.3e-14
assert 8 * LIN_WORST_MEASURED <= LIN_BOUND <= 1e-12


# ---- residual functions (mpmath) -------------------------------------------------------------------
def _mp():
    import mpmath
    return mpmath


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _rotate(w, X):
    """X turned by the axis-angle vector w, through the unit quaternion (cos th/2, sin th/2 * w / th)"""
    mp = _mp()
    th = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th == 0:
        return list(X)
    q0, s = mp.cos(th / 2), mp.sin(th / 2) / th
    q = [s * w[0], s * w[1], s * w[2]]
    c1 = _cross(q, X)
    c2 = _cross(q, c1)
    return [X[i] + 2 * (q0 * c1[i] + c2[i]) for i in range(3)]


def _project(P, f, k1, k2):
    px, py = -P[0] / P[2], -P[1] / P[2]
    r2 = px * px + py * py
    d = f * (1 + r2 * (k1 + k2 * r2))
    return [d * px, d * py]


def residual_bal9(cam, pt, xy):
    """cam = [w(3), t(3), f, k1, k2], pt (3), xy (2), all mpf -> residual (2)"""
    P = _rotate(cam[0:3], pt)
    P = [P[i] + cam[3 + i] for i in range(3)]
    p = _project(P, cam[6], cam[7], cam[8])
    return [p[0] - xy[0], p[1] - xy[1]]


def residual_se3(cam, pt, xy, delta, dX):
    """the residual after T <- exp(delta) T (delta = translation part, rotation part) and X <- X + dX;
    a point in front of the image plane (camera-frame z > 0.01) gives (25, 0)"""
    mp = _mp()
    X = [pt[i] + dX[i] for i in range(3)]
    P = _rotate(cam[0:3], X)
    P = [P[i] + cam[3 + i] for i in range(3)]
    u, w = delta[0:3], delta[3:6]
    P = _rotate(w, P)
    th = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th == 0:
        Vu = list(u)
    else:  # V u = u + (1 - cos th) / th^2  w x u + (th - sin th) / th^3  w x (w x u)
        wu = _cross(w, u)
        wwu = _cross(w, wu)
        a, b = (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3
        Vu = [u[i] + a * wu[i] + b * wwu[i] for i in range(3)]
    P = [P[i] + Vu[i] for i in range(3)]
    if P[2] > mp.mpf(0.01):
        return [mp.mpf(25), mp.mpf(0)]
    p = _project(P, cam[6], cam[7], cam[8])
    return [p[0] - xy[0], p[1] - xy[1]]


def _central(fn, nvar, h):
    """(2, nvar) central differences of fn(list of nvar offsets) at 0"""
    mp = _mp()
    out = []
    for i in range(nvar):
        d = [mp.mpf(0)] * nvar
        d[i] = h
        rp = fn(d)
        d[i] = -h
        rm = fn(d)
        out.append([(rp[e] - rm[e]) / (2 * h) for e in range(2)])
    return [[out[i][e] for i in range(nvar)] for e in range(2)]


def linearize_one(param, cam, pt, xy, step_exp=STEP_EXP):
    """one observation: (residual (2), J (2 x 12 for bal9: camera 0..8, point 9..11; 2 x 9 for se3:
    delta 0..5, point 6..8), projection (2)) as mpf lists"""
    mp = _mp()
    with mp.workdps(DPS):
        cam = [mp.mpf(float(v)) for v in cam]
        pt = [mp.mpf(float(v)) for v in pt]
        xy = [mp.mpf(float(v)) for v in xy]
        h = mp.mpf(10) ** step_exp
        zero3 = [mp.mpf(0)] * 3
        if param == "bal9":
            r = residual_bal9(cam, pt, xy)
            J = _central(lambda d: residual_bal9([cam[i] + d[i] for i in range(9)],
                                                 [pt[i] + d[9 + i] for i in range(3)], xy), 12, h)
        else:
            r = residual_se3(cam, pt, xy, [mp.mpf(0)] * 6, zero3)
            J = _central(lambda d: residual_se3(cam, pt, xy, d[0:6], d[6:9]), 9, h)
        return r, J, [r[0] + xy[0], r[1] + xy[1]]


# ---- linearisation cases ---------------------------------------------------------------------------
def _scene(num_cams=6, num_pts=12, seed=2):
    from baspacho_amd import bal
    return bal.synth_scene(num_cams, num_pts, seed=seed)


def _scaled(min_theta):
    """synth_scene(6, 12, seed=2) with every rotation scaled so that the smallest angle is min_theta"""
    from baspacho_amd import bal
    p = _scene()
    cams = p.cams.copy()
    cams[:, 0:3] *= min_theta / np.linalg.norm(cams[:, 0:3], axis=1).min()
    return bal.BalProblem(cams, p.pts, p.obs_cam, p.obs_pt, p.obs_xy)


def _with_theta2(w, th2):
    w = np.asarray(w, dtype=np.float64)
    return w * np.sqrt(th2 / float(w @ w))


def _special():
    """one camera per rotation edge, each seeing three points; and a camera turned about its own z axis
    with three points at camera-frame z = +5, 0.011 and 0.009 (exact: the rotation leaves z alone and the
    translation has no z)"""
    from baspacho_amd import bal
    base = _scene()
    axis = np.array([0.3, -0.5, 0.8])
    rot = [_with_theta2(axis, BAL9_CUT * (1 + 1e-6)), _with_theta2(axis, BAL9_CUT * (1 - 1e-6)),
           _with_theta2(axis, SE3_CUT * 1.01), _with_theta2(axis, SE3_CUT * 0.99),
           np.zeros(3), np.array([1e-170, 0.0, 0.0]), np.array([0.3, 0.0, -0.2]),
           _with_theta2(axis, 3.1 ** 2), _with_theta2(axis, 4.0 ** 2)]
    assert rot[0] @ rot[0] > BAL9_CUT > rot[1] @ rot[1] and rot[2] @ rot[2] > SE3_CUT > rot[3] @ rot[3]
    assert rot[5] @ rot[5] == 0.0, "theta^2 of (1e-170, 0, 0) underflows"
    cams = np.tile(base.cams[0], (len(rot) + 1, 1))
    cams[:len(rot), 0:3] = rot
    cams[-1, 0:6] = (0.0, 0.0, 0.3, 1e-3, -2e-3, 0.0)
    pts = np.concatenate([base.pts[:3], [[2e-3, 1e-3, 5.0], [2e-3, 1e-3, 0.011], [2e-3, 1e-3, 0.009]]])
    oc = np.concatenate([np.repeat(np.arange(len(rot)), 3), [len(rot)] * 3]).astype(np.int64)
    op = np.concatenate([np.tile(np.arange(3), len(rot)), [3, 4, 5]]).astype(np.int64)
    xy = bal.project(base.cams[np.zeros(len(oc), dtype=np.int64)], base.pts[op % 3]) + 0.5
    return bal.BalProblem(cams, pts, oc, op, xy)


def _generic():
    """65 observations of a generic scene: its prefixes of 1, 63 and 64 are the launch-size cases"""
    from baspacho_amd import bal
    p = _scene(6, 24, 2)
    assert len(p.obs_cam) >= 65
    return bal.BalProblem(p.cams, p.pts, p.obs_cam[:65], p.obs_pt[:65], p.obs_xy[:65])


LIN_CASES = {"generic": _generic, "theta1e-3": lambda: _scaled(1e-3), "theta1e-5": lambda: _scaled(1e-5),
             "theta1e-7": lambda: _scaled(1e-7), "theta1e-9": lambda: _scaled(1e-9), "special": _special}
OBS_COUNTS = (1, 63, 64, 65)
SPECIAL_Z = {-3: 5.0, -2: 0.011, -1: 0.009}   # the last three observations of "special"
_PROBLEMS, _REFS = {}, {}


def lin_problem(name):
    if name not in _PROBLEMS:
        p = LIN_CASES[name]()
        assert len(p.obs_cam) <= 70
        _PROBLEMS[name] = p
    return _PROBLEMS[name]


def lin_reference(name, param, step_exp=STEP_EXP):
    """(res (n, 2), Jc (n, 2, cs), Jp (n, 2, 3), projection (n, 2)) of the named case, rounded to float64
    from the mpmath values; computed once per process"""
    key = (name, param, step_exp)
    if key not in _REFS:
        p = lin_problem(name)
        cs = 9 if param == "bal9" else 6
        n = len(p.obs_cam)
        res, J, proj = np.zeros((n, 2)), np.zeros((n, 2, cs + 3)), np.zeros((n, 2))
        for o in range(n):
            r, Jo, pr = linearize_one(param, p.cams[p.obs_cam[o]], p.pts[p.obs_pt[o]], p.obs_xy[o], step_exp)
            res[o] = [float(v) for v in r]
            proj[o] = [float(v) for v in pr]
            J[o] = [[float(v) for v in row] for row in Jo]
        for a in (res, J, proj):
            a.setflags(write=False)
        _REFS[key] = (res, J[:, :, :cs], J[:, :, cs:], proj)
    return _REFS[key]


def lin_errors(got, ref):
    """worst scaled errors of (res, Jc, Jp) against lin_reference's tuple: the residual by
    |projection|_inf + |xy|_inf of its observation, every Jacobian entry by the larger of the two entries of
    its column in its observation.  A column the reference has as exactly zero must be exactly zero
    (error inf otherwise).  Returns (residual error, Jacobian error)."""
    res, Jc, Jp = (np.asarray(a, dtype=np.float64) for a in got)
    rres, rJc, rJp, proj = ref
    n = len(rres)
    res, Jc, Jp = res.reshape(n, 2), Jc.reshape(n, 2, -1), Jp.reshape(n, 2, 3)
    xy = proj - rres
    scale = np.abs(proj).max(axis=1) + np.abs(xy).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        eres = np.abs(res - rres).max(axis=1) / scale
        worst = 0.0
        for J, rJ in ((Jc, rJc), (Jp, rJp)):
            col = np.abs(rJ).max(axis=1, keepdims=True)
            e = np.abs(J - rJ) / col
            e = np.where(col == 0, np.where(J == 0, 0.0, np.inf), e)
            e = np.where(np.isfinite(J), e, np.inf)
            worst = max(worst, float(e.max()))
    eres = np.where(np.isfinite(res).all(axis=1), eres, np.inf)
    return float(eres.max()), worst


# ---- dense normal equations --------------------------------------------------------------------------
def dense_jacobian(num_pts, num_cams, cam_size, obs_cam, obs_pt, Jc, Jp):
    """J (2 nobs x order) in the caller's parameter order: points (3 each) first, then cameras"""
    n = len(obs_cam)
    J = np.zeros((2 * n, 3 * num_pts + cam_size * num_cams))
    for o in range(n):
        p0, c0 = 3 * int(obs_pt[o]), 3 * num_pts + cam_size * int(obs_cam[o])
        J[2 * o:2 * o + 2, p0:p0 + 3] += Jp[o]
        J[2 * o:2 * o + 2, c0:c0 + cam_size] += Jc[o]
    return J


def normal_equations(num_pts, num_cams, cam_size, obs_cam, obs_pt, Jc, Jp, res):
    """H = J^T J and g = J^T r in np.longdouble from the dense J, with A = sum |J_a| |J_b|, the number N of
    observations that contribute to each element (one term per observation: its two rows are summed before
    they reach the matrix) and the same pair (Ag, Ng) for g; all in the caller's order.  Observation by
    observation, so that the cost is that of the blocks and not of a dense product; an observation counts
    on all 3 + cam_size columns of its two parameters, zero Jacobian entries included (the kernel adds the
    zero)."""
    J = dense_jacobian(num_pts, num_cams, cam_size, obs_cam, obs_pt, Jc, Jp)
    n = J.shape[1]
    mask = np.zeros((len(obs_cam), n), dtype=bool)
    for o in range(len(obs_cam)):
        p0, c0 = 3 * int(obs_pt[o]), 3 * num_pts + cam_size * int(obs_cam[o])
        mask[o, p0:p0 + 3] = True
        mask[o, c0:c0 + cam_size] = True
    L = np.longdouble
    H, A, N = np.zeros((n, n), dtype=L), np.zeros((n, n), dtype=L), np.zeros((n, n), dtype=np.int64)
    g, Ag, Ng = np.zeros(n, dtype=L), np.zeros(n, dtype=L), np.zeros(n, dtype=np.int64)
    r = np.asarray(res, dtype=L).reshape(-1, 2)
    for o in range(len(obs_cam)):
        idx = np.nonzero(mask[o])[0]
        Jo = J[2 * o:2 * o + 2][:, idx].astype(L)
        sel = np.ix_(idx, idx)
        H[sel] += Jo.T @ Jo
        A[sel] += np.abs(Jo).T @ np.abs(Jo)
        N[sel] += 1
        g[idx] += Jo.T @ r[o]
        Ag[idx] += np.abs(Jo).T @ np.abs(r[o])
        Ng[idx] += 1
    return {"J": J, "H": H, "g": g, "A": A, "N": N, "Ag": Ag, "Ng": Ng}


def layout(sol, num_pts, num_cams, cam_size):
    """how the caller's dense order reaches the solver's numeric layout, from the skeleton and
    scalarPermutation() alone: (rows, cols) = the caller-order dense position of every data element, `lower`
    = the element lies in a block the pipeline writes if an observation links its two parameters (the
    row's span is not before the column's: off-diagonal blocks once, diagonal blocks in full), `diag` = the
    data index of every scalar's diagonal element (caller's order), `vec` = the position of every caller
    scalar in an internal-order vector"""
    from autograd_ref import element_coords
    n = sol.order()
    assert n == 3 * num_pts + cam_size * num_cams
    sp = sol.scalarPermutation()
    inv = np.empty(n, dtype=np.int64)
    inv[sp] = np.arange(n)
    ri, ci = element_coords(sol)
    span_of = np.searchsorted(sol.skel()["spanStart"], np.arange(n), side="right") - 1
    lower = span_of[ri] >= span_of[ci]
    on_diag = np.nonzero(ri == ci)[0]
    diag = np.empty(n, dtype=np.int64)
    diag[inv[ri[on_diag]]] = on_diag
    assert len(on_diag) == n
    return {"rows": inv[ri], "cols": inv[ci], "lower": lower, "diag": diag, "vec": sp}


# ---- Hessian-fill scenes ---------------------------------------------------------------------------
def _all_see_all(nc, npt):
    return np.repeat(np.arange(nc), npt), np.tile(np.arange(npt), nc)


def _fill_problem(name):
    """(BalProblem, elimination ranges: None = those of bal_structure, () = none given)"""
    from baspacho_amd import bal
    if name in ("40x6", "37x5", "9x9"):
        nc, npt = (int(v) for v in name.split("x"))
        return bal.synth_scene_for(nc, npt, *_all_see_all(nc, npt)), ()
    if name == "30x8":   # camera c sees points c, c + 1, c + 2 (mod 8)
        oc = np.repeat(np.arange(30), 3)
        return bal.synth_scene_for(30, 8, oc, (oc + np.tile(np.arange(3), 30)) % 8), ()
    if name == "16x400":
        return bal.synth_scene(16, 400), None
    if name == "64x1":
        return bal.synth_scene_for(64, 1, *_all_see_all(64, 1)), None
    if name == "1x300":
        return bal.synth_scene_for(1, 300, *_all_see_all(1, 300)), None
    if name == "dup7":   # 7 observations a second and a third time, under other xy
        p = bal.synth_scene(5, 30, seed=4)
        rep = np.array([0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 4, 5, 6])
        xy = np.concatenate([p.obs_xy, p.obs_xy[rep] + np.linspace(-3, 3, 28).reshape(14, 2)])
        return bal.BalProblem(p.cams, p.pts, np.concatenate([p.obs_cam, p.obs_cam[rep]]),
                              np.concatenate([p.obs_pt, p.obs_pt[rep]]), xy), None
    raise KeyError(name)


FILL_SCENES = ("40x6", "37x5", "30x8", "9x9", "16x400", "64x1", "1x300", "dup7")
# observations, and how many of them the accessor answers flipped = 1 for (9-wide cameras, Settings())
FLIPPED = {"40x6": (240, 204), "37x5": (185, 160), "30x8": (90, 90), "9x9": (81, 72)}
_FILL = {}


def fill_case(name, cam_size):
    """dict of the named scene at the camera size: prob, sol, Jc / Jp / res of the host model (float64;
    the fill's inputs), ne = normal_equations of them, lay = layout(sol); built once per process"""
    key = (name, cam_size)
    if key not in _FILL:
        import baspacho_amd as B
        from baspacho_amd import bal
        from oracle import bal_model
        prob, ranges = _fill_problem(name)
        sizes, ss, auto = bal.bal_structure(prob, cam_size=cam_size)
        sol = B.create_solver(B.Settings(), sizes, ss, auto if ranges is None else ranges)
        lin = bal_model.linearize if cam_size == 9 else bal_model.linearize_se3
        res, Jc, Jp = lin(prob.cams[prob.obs_cam], prob.pts[prob.obs_pt], prob.obs_xy)
        c = {"prob": prob, "sol": sol, "res": res, "Jc": Jc, "Jp": Jp, "cam_size": cam_size,
             "ne": normal_equations(prob.num_pts, prob.num_cams, cam_size, prob.obs_cam, prob.obs_pt, Jc, Jp, res),
             "lay": layout(sol, prob.num_pts, prob.num_cams, cam_size)}
        _FILL[key] = c
    return _FILL[key]


def expected_fill(ne, lay, dtype):
    """per data element and per vector entry of the solver's layout: (H, bound, touched) and
    (g, bound, touched).  bound = 2 (n + 1) eps_T sum |J_a| |J_b|: each of the n terms is rounded once to T
    and takes part in at most n atomic additions, in any order, onto a prior no larger than that sum."""
    eps = np.longdouble(np.finfo(dtype).eps)
    r, c = lay["rows"], lay["cols"]
    touched = (ne["N"][r, c] > 0) & lay["lower"]
    H = np.where(touched, ne["H"][r, c], 0)
    bound = np.where(touched, 2 * (ne["N"][r, c] + 1) * eps * ne["A"][r, c], 0)
    A = np.where(touched, ne["A"][r, c], 0)
    n = len(ne["g"])
    g, gb, gt, gA = (np.zeros(n, dtype=np.longdouble), np.zeros(n, dtype=np.longdouble), np.zeros(n, dtype=bool),
                     np.zeros(n, dtype=np.longdouble))
    g[lay["vec"]] = ne["g"]
    gb[lay["vec"]] = 2 * (ne["Ng"] + 1) * eps * ne["Ag"]
    gt[lay["vec"]] = ne["Ng"] > 0
    gA[lay["vec"]] = ne["Ag"]
    return {"H": H, "Hbound": bound, "Htouched": touched, "HA": A, "g": g, "gbound": gb, "gtouched": gt, "gA": gA}


def prior_for(exp, dtype, seed):
    """a random prior for data and grad: every touched element gets a value no larger than its own sum of
    absolute products (the bound has no term for the prior, so the prior must not outweigh what is added to
    it), every other element a value in (-1, 1)"""
    rng = np.random.default_rng(seed)
    out = []
    for A, touched in ((exp["HA"], exp["Htouched"]), (exp["gA"], exp["gtouched"])):
        u = rng.uniform(-1, 1, len(A))
        out.append(np.where(touched, u * A.astype(np.float64), u).astype(dtype))
    return out
