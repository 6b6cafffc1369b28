"""The BAL reference of tests/bal_ref.py against itself, the host model (oracle/bal_model.py) against the
reference, and proof that the comparison sees the defect it was written for.

Measured here (float64 host model against the 70-digit reference, worst over the whole linearisation case
list of bal_ref.LIN_CASES; Jacobians scaled per observation and column, residuals by |projection| + |xy|):

    bal9   residual 3.1e-16   Jacobian 1.03e-14  (case "special"; 1.3e-15 .. 3.3e-15 on the scaled scenes)
    se3    residual 3.1e-16   Jacobian 1.03e-15

LIN_BOUND = 8 x the worst of these = 8.3e-14 is what tests/test_bal_edges_gpu.py holds the kernels to (the
factor 8 allows for fma contraction and the device's sin / cos).  It has to stay below 1e-12: the defect of
the earlier k = w / theta formula sits at 1e-9 .. 4e-8."""
import numpy as np
import pytest

import bal_ref as R
from oracle import bal_model

WORST_MEASURED, LIN_BOUND = R.LIN_WORST_MEASURED, R.LIN_BOUND   # recorded in bal_ref.py, shared with the GPU tests
assert (WORST_MEASURED, LIN_BOUND) == (1.03e-14, 8.3e-14)


def test_reference_agrees_with_itself():
    """central differences at steps 1e-25 and 1e-24 differ by less than 1e-20 (absolute, on Jacobian
    entries of size up to 1e5): neither truncation nor rounding is near the 1e-25 the reference claims"""
    import mpmath as mp
    for name, obs in (("special", range(30)), ("theta1e-9", range(0, 30, 5)), ("generic", range(0, 65, 13))):
        p = R.lin_problem(name)
        for param in ("bal9", "se3"):
            for o in obs:
                args = (param, p.cams[p.obs_cam[o]], p.pts[p.obs_pt[o]], p.obs_xy[o])
                _, Ja, _ = R.linearize_one(*args, step_exp=-25)
                _, Jb, _ = R.linearize_one(*args, step_exp=-24)
                with mp.workdps(R.DPS):
                    worst = max(abs(a - b) for ra, rb in zip(Ja, Jb) for a, b in zip(ra, rb))
                    assert worst < mp.mpf(10) ** -20, (name, param, o, worst)


def test_se3_reference_applies_the_behind_the_camera_rule():
    res, Jc, Jp, _ = R.lin_reference("special", "se3")
    for o, z in R.SPECIAL_Z.items():
        bad = z > 0.01
        assert (tuple(res[o]) == (25.0, 0.0)) == bad
        assert (not Jc[o].any() and not Jp[o].any()) == bad


def _model_errors():
    out = {}
    for param, fn in (("bal9", bal_model.linearize), ("se3", bal_model.linearize_se3)):
        for name in R.LIN_CASES:
            p = R.lin_problem(name)
            out[param, name] = R.lin_errors(fn(p.cams[p.obs_cam], p.pts[p.obs_pt], p.obs_xy),
                                            R.lin_reference(name, param))
    return out


def test_host_model_against_the_reference():
    """the number LIN_BOUND is taken from, printed per case.  The host model must stay where it was measured:
    within a factor 2 of the recorded worst error (numpy's sin / cos differ in the last bit between builds)"""
    errs = _model_errors()
    for key, (eres, ejac) in errs.items():
        print("%-5s %-10s residual %.2e  Jacobian %.2e" % (key + (eres, ejac)))
    worst = max(max(e) for e in errs.values())
    print("worst %.3e, bound %.3e" % (worst, LIN_BOUND))
    assert worst <= 2 * WORST_MEASURED


def _axis_form_jacobian(cams, pts, xy):
    """the bal9 rotation as reproject() had it before: axis k = w / theta in the dual path"""
    D = bal_model.Dual
    n = len(cams)
    w, t = [D.var(cams[:, i], i) for i in range(3)], [D.var(cams[:, 3 + i], 3 + i) for i in range(3)]
    X = [D.var(pts[:, i], 9 + i) for i in range(3)]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = np.sqrt(th2.v)
    theta = th2.fn(th, 0.5 / th)
    c, s = theta.fn(np.cos(th), -np.sin(th)), theta.fn(np.sin(th), np.cos(th))
    k = [wi / theta for wi in w]
    kx = [k[1] * X[2] - k[2] * X[1], k[2] * X[0] - k[0] * X[2], k[0] * X[1] - k[1] * X[0]]
    kdot = (k[0] * X[0] + k[1] * X[1] + k[2] * X[2]) * (D.const(np.ones(n)) - c)
    P = [X[i] * c + kx[i] * s + k[i] * kdot + t[i] for i in range(3)]
    J = np.stack([((D.const(np.zeros(n)) - P[e]) / P[2]).d for e in range(2)], axis=1)
    return J   # d(-P.xy / P.z): the distortion only scales it


def test_the_comparison_sees_the_one_over_theta_defect():
    """at theta = 1e-7 the earlier formula misses the reference by 1e-9 (column-scaled), more than 100 x the
    bound; the restated one does not"""
    p = R.lin_problem("theta1e-7")
    cams, pts = p.cams[p.obs_cam].copy(), p.pts[p.obs_pt]
    cams[:, 6], cams[:, 7:9] = 1.0, 0.0   # f = 1, no distortion: the residual is -P.xy / P.z - xy
    old = _axis_form_jacobian(cams, pts, p.obs_xy)
    _, Jc, Jp = bal_model.linearize(cams, pts, p.obs_xy)
    new = np.concatenate([Jc, Jp], axis=2)
    ref = np.zeros_like(new)
    for o in range(len(cams)):
        _, Jo, _ = R.linearize_one("bal9", cams[o], pts[o], p.obs_xy[o])
        ref[o] = [[float(v) for v in row] for row in Jo]
    keep = [0, 1, 2, 3, 4, 5, 9, 10, 11]   # f, k1, k2 columns: not part of the copied formula
    col = np.abs(ref).max(axis=1, keepdims=True)

    def err(J):
        return float((np.abs(J - ref) / col)[:, :, keep].max())
    print("earlier formula %.2e, restated %.2e, bound %.1e" % (err(old), err(new), LIN_BOUND))
    assert err(old) > 100 * LIN_BOUND
    assert err(new) <= LIN_BOUND / 8


@pytest.mark.parametrize("name,cam_size", [("40x6", 9), ("9x9", 6), ("dup7", 9)])
def test_dense_layout_mapping_agrees_with_the_accessor_walk(name, cam_size):
    """the expected values of the GPU fill tests come from dense J^T J, the skeleton and scalarPermutation();
    here that path is cross-checked once against the accessor-driven host assembly (which produces none of
    the expected values): same touched set, same numbers to rounding"""
    c = R.fill_case(name, cam_size)
    sol, prob = c["sol"], c["prob"]
    exp = R.expected_fill(c["ne"], c["lay"], np.float64)
    if cam_size == 9:
        data, grad, offs = bal_model.fill_hessian_host(sol, prob, c["Jc"], c["Jp"], c["res"], 0.0)
        if name in R.FLIPPED:
            assert (len(offs), int(offs[:, 2].sum())) == R.FLIPPED[name]
    else:
        data, grad = bal_model.fill_hessian_host_se3(sol, prob, c["Jc"], c["Jp"], c["res"], 0.0)
    assert np.all(np.abs(data - exp["H"]) <= exp["Hbound"])
    assert not data[~exp["Htouched"]].any()
    assert np.all(np.abs(grad - exp["g"]) <= exp["gbound"])
    # damping formula on the diagonal elements the layout names
    lam = 0.3
    if cam_size == 9:
        damped, _, _ = bal_model.fill_hessian_host(sol, prob, c["Jc"], c["Jp"], c["res"], lam)
    else:
        damped, _ = bal_model.fill_hessian_host_se3(sol, prob, c["Jc"], c["Jp"], c["res"], lam)
    d = c["lay"]["diag"]
    changed = np.nonzero(damped != data)[0]
    assert set(changed.tolist()) <= set(d.tolist())
    assert np.allclose(damped[d], data[d] * (1 + lam) + 1e-3 * lam, rtol=1e-15, atol=0)
