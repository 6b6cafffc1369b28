"""The reference of tests/bal_step_ref.py against itself, its float64 host models against the reference (the
measurement the GPU bounds are taken from), and the host LM against the end-to-end conditions.

Measured here (float64 host models against mpmath at 70 digits):

    retraction over STEP_CASES   max |R(w_out) - R_ref| 3.4e-16 ("lands 1e-3 past pi")
                                 |t_out - t_ref| / (|t| + |u|) 1.6e-16 ("step rotation 3.0")
    loss over loss_cases(2.0)    rho 2.2e-16 (Huber), sqrt(w) 1.3e-16, scaled words 2.3e-16 (Cauchy)

STEP_BOUND_R = 2.7e-15, STEP_BOUND_T = 1.3e-15 and LOSS_BOUND = 1.8e-15 (8.3 eps) are 8 x these; the caps are
1e-13 and 64 eps.  The host path misses the rotation by 1e-9 near pi (so3_log) and the translation by 1e-10 at a
step rotation of 1e-9 (se3_exp), which is what the caps keep out."""
import os
import re

import numpy as np
import pytest

import bal_ref as R
import bal_step_ref as S
from baspacho_amd import _lib, bal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bsp_bal_residuals_f64", "bsp_bal_residuals_se3_f64", "bsp_bal_loss_f64", "bsp_bal_sum_f64",
               "bsp_bal_sum_scratch_len", "bsp_bal_apply_step_f64", "bsp_bal_apply_step_se3_f64"]


def test_new_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        hdr = f.read()
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t) %s\(" % n, hdr), n
        assert hasattr(lib, n), n
    assert [int(lib.bsp_bal_sum_scratch_len(n)) for n in (0, 1, 2048, 2049)] == [0, 1, 1, 2]
    for name in ("residuals", "apply_loss", "cost", "cost_linearized", "apply_step", "set_params", "to_problem"):
        assert callable(getattr(bal.DevicePipeline, name)), name
    assert callable(bal.lm_optimize_device)


def test_bounds_are_tied_to_the_measurements():
    assert S.STEP_BOUND_R == 8 * S.STEP_WORST_R_MEASURED <= 1e-13
    assert S.STEP_BOUND_T == 8 * S.STEP_WORST_T_MEASURED <= 1e-13
    assert S.LOSS_BOUND == 8 * S.LOSS_WORST_MEASURED <= 64 * S.EPS


# ---- loss reference ------------------------------------------------------------------------------------
def test_loss_reference_derivative_is_the_difference_quotient_of_rho():
    """rho' against central differences of rho (step 1e-25, as in bal_ref) away from the Huber kink, and
    against one-sided differences on each side of it"""
    import mpmath as mp
    with mp.workdps(S.DPS):
        h, a = mp.mpf(10) ** R.STEP_EXP, mp.mpf(2)
        tol = mp.mpf(10) ** -20
        for kind in ("trivial", "huber", "cauchy"):
            for s in (mp.mpf("1e-3"), mp.mpf("0.7"), mp.mpf("3.9"), mp.mpf("4.1"), mp.mpf(625), mp.mpf("1e6")):
                fd = (S.rho_mp(kind, a, s + h) - S.rho_mp(kind, a, s - h)) / (2 * h)
                assert abs(fd - S.drho_mp(kind, a, s)) < tol, (kind, s)
        kink = a * a
        below = (S.rho_mp("huber", a, kink) - S.rho_mp("huber", a, kink - h)) / h
        above = (S.rho_mp("huber", a, kink + 2 * h) - S.rho_mp("huber", a, kink + h)) / h
        assert abs(below - 1) < tol and S.drho_mp("huber", a, kink) == 1   # the strict > of SoftLoss.h
        assert abs(above - S.drho_mp("huber", a, kink + h)) < tol and above < 1
        assert S.rho_mp("huber", a, kink) == kink                          # rho is continuous at the kink
        assert abs(S.rho_mp("huber", a, kink + h) - kink - h) < tol * h


# ---- retraction reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cam,step", S.STEP_CASES, ids=[n.replace(" ", "_") for n in S.STEP_NAMES])
def test_retraction_reference_is_the_parameterisation_the_linearisation_differentiates(name, cam, step):
    """residual_se3(cam, pt, xy, delta = -step_cam, dX = -step_pt) == the residual at the retracted camera
    (R', t') and point, to 1e-60"""
    import mpmath as mp
    rng = np.random.default_rng(len(name))
    with mp.workdps(S.DPS):
        Rc = np.array(S.rotation_mp([S._f(v) for v in cam[0:3]]).tolist(), dtype=np.float64)
        Rn, tn = S.retract_se3_mp(cam, step)
        hit = 0
        for _ in range(3):
            pt = Rc.T @ (np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), -10.0]) - cam[3:6])   # 10 in front
            dpt, xy = 1e-2 * rng.standard_normal(3), rng.uniform(-300, 300, 2)
            mcam, mpt, mxy = [S._f(v) for v in cam], [S._f(v) for v in pt], [S._f(v) for v in xy]
            want = R.residual_se3(mcam, mpt, mxy, [-S._f(v) for v in step], [-S._f(v) for v in dpt])
            X = mp.matrix([mpt[i] - S._f(dpt[i]) for i in range(3)])
            P = Rn * X + tn
            if P[2] > mp.mpf(0.01):
                got = [mp.mpf(25), mp.mpf(0)]
            else:
                p = R._project([P[0], P[1], P[2]], mcam[6], mcam[7], mcam[8])
                got = [p[0] - mxy[0], p[1] - mxy[1]]
                hit += 1
            for g, w in zip(got, want):
                assert abs(g - w) <= mp.mpf(10) ** -60 * (1 + abs(w)), (name, g, w)
        assert hit > 0 or "3.0" in name or "pi" in name


# ---- the yardsticks --------------------------------------------------------------------------------------
def test_retraction_model_against_the_reference():
    """the numbers STEP_BOUND_R / STEP_BOUND_T are taken from, printed per case; the model must stay where it
    was measured (within a factor 2: numpy's sin / cos differ in the last bit between builds)"""
    out = S.retract_se3_model(S.STEP_CAMS, S.STEP_STEPS)
    eR, eT = S.step_errors(S.STEP_CAMS, S.STEP_STEPS, out)
    for n, a, b in zip(S.STEP_NAMES, eR, eT):
        print("%-45s R %.2e  t %.2e" % (n, a, b))
    print("worst R %.3e (recorded %.1e)  t %.3e (recorded %.1e)" % (eR.max(), S.STEP_WORST_R_MEASURED, eT.max(),
                                                                    S.STEP_WORST_T_MEASURED))
    assert eR.max() <= 2 * S.STEP_WORST_R_MEASURED and eT.max() <= 2 * S.STEP_WORST_T_MEASURED
    assert np.all(np.linalg.norm(out[:, 0:3], axis=1) <= np.pi * (1 + 4 * S.EPS))
    assert np.array_equal(out[:, 6:9], S.STEP_CAMS[:, 6:9])
    i = S.STEP_NAMES.index("lands 1e-3 past pi")   # canonical output: angle pi - 1e-3 about the flipped axis
    assert abs(np.linalg.norm(out[i, 0:3]) - (np.pi - 1e-3)) < 1e-12 and out[i, 0:3] @ S.STEP_CAMS[i, 0:3] < 0
    i = S.STEP_NAMES.index("zero step")
    assert np.allclose(out[i], S.STEP_CAMS[i], rtol=4 * S.EPS, atol=0)


def test_the_comparison_sees_the_two_defects_of_the_host_path():
    """bal.se3_exp / so3_exp / so3_log (the path of apply_step_se3, pinned as it is by the existing tests): the
    rotation of the cases that land near pi is off by 1e-9 (acos of the trace), the translation of the
    1e-9 step by 1e-10 ((1 - cos th) / th^2 in closed form) -- both far outside the caps on the bounds"""
    out = S.STEP_CAMS.copy()
    for i in range(len(out)):
        Rd, td = bal.se3_exp(-S.STEP_STEPS[i])
        out[i, 0:3] = bal.so3_log(Rd @ bal.so3_exp(S.STEP_CAMS[i, 0:3]))
        out[i, 3:6] = Rd @ S.STEP_CAMS[i, 3:6] + td
    eR, eT = S.step_errors(S.STEP_CAMS, S.STEP_STEPS, out)
    near_pi = [i for i, n in enumerate(S.STEP_NAMES) if n.startswith("lands")]
    tiny = S.STEP_NAMES.index("step rotation 1e-9")
    print("host path: R near pi %s, t at 1e-9 %.1e" % (", ".join("%.1e" % e for e in eR[near_pi]), eT[tiny]))
    assert eR[near_pi].max() > 1e-13 and eT[tiny] > 1e-13


@pytest.mark.parametrize("kind", ["trivial", "huber", "cauchy"])
def test_loss_model_against_the_reference(kind):
    """the number LOSS_BOUND is taken from: rho, sqrt(w) and the scaled words of the float64 model"""
    import mpmath as mp
    a = 2.0
    res, fixed = S.loss_cases(a, 65, seed=S.KINDS[kind])
    rho, sq = S.loss_model(kind, a, res)
    J = np.random.default_rng(5).uniform(-50, 50, (65, 18))
    J[fixed] = 0.0
    e_rho, e_w = S.loss_errors(kind, a, res, rho, [(res, res * sq[:, None]), (J, J * sq[:, None])])
    with mp.workdps(S.DPS):
        e_sq = max(S._rel(g, w) for g, w in zip(sq, S.loss_reference(kind, a, res)[1]))
    print("%s: rho %.2e sqrt(w) %.2e words %.2e (recorded %.1e)" % (kind, e_rho, e_sq, e_w, S.LOSS_WORST_MEASURED))
    assert max(e_rho, e_sq, e_w) <= 2 * S.LOSS_WORST_MEASURED
    unit = S.unit_weight(kind, a, res)
    assert np.all(sq[unit] == 1.0) and unit.any()
    assert kind == "trivial" or (~unit).any()


def test_sum_model_is_a_sum():
    rng = np.random.default_rng(2)
    for n in (0, 1, 255, 2047, 2048, 2049, 2048 * 256 + 1):
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
        got, want = S.sum_model(x, 0.5), 0.5 * float(np.sum(x.astype(np.longdouble)))
        assert abs(got - want) <= 32 * S.EPS * 0.5 * float(np.abs(x).sum()), n   # a tree of depth <= 26 + 8
    assert S.sum_model(np.zeros(0), -3.0) == 0.0 and not np.signbit(S.sum_model(np.zeros(0), -3.0))


# ---- host LM ---------------------------------------------------------------------------------------------
def test_host_lm_meets_the_end_to_end_conditions():
    """on the outlier scene (5 % of the observations off by 40 .. 80 px) the trivial loss ends far above the
    inlier noise floor, Huber(2) far below the trivial result, Cauchy(2) at the floor; without outliers the
    trivial loss meets the conditions of the LM test of tests/test_bal_gpu.py"""
    prob, inlier = S.outlier_scene(3)
    floor = S.noise_floor(int(inlier.sum()))
    end = {}
    for loss in (None, ("huber", 2.0), ("cauchy", 2.0)):
        out, hist = S.lm_host(prob, loss)
        end[loss and loss[0]] = S.inlier_cost(out, inlier)
        print("%s: inlier cost %.1f = %.2f x floor after %d iterations" % (loss, end[loss and loss[0]],
                                                                          end[loss and loss[0]] / floor, len(hist)))
    assert end[None] > 20 * floor
    assert end["huber"] < 0.2 * end[None]
    assert end["cauchy"] < 2 * floor
    clean = bal.synth_scene(14, 300, seed=3, perturb=2e-2)
    cost0 = bal.total_cost(clean)
    out, hist = S.lm_host(clean, None, max_iters=25)
    cost1 = bal.total_cost(out)
    assert cost1 < 0.02 * cost0 and cost1 < 2 * S.noise_floor(len(clean.obs_cam))
    assert len([h for h in hist if h[1] <= h[0]]) >= 3
