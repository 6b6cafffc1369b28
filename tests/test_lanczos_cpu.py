"""CPU: the numpy restatement of the device-resident Lanczos recurrence (lanczos_ref.py)
against dense numpy (V^T A V, orthogonality, the exact log-determinant from identity probes, the residual
bounds of the Ritz values on the analytic Toeplitz spectrum), every stop reason reached by a named input, the
host post-processing on a closed-form tridiagonal, the subtraction order of the projection, and the argument
refusals of the bsp_lanczos_* entries.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from baspacho_amd import _lib
from baspacho_amd import lanczos as L
from baspacho_amd import sparse as S
import cg_ref as R
import lanczos_ref as LR
import sym_product_ref as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = ("init", "alpha", "update", "project", "subtract", "normalize")
SYMBOLS = ["bsp_lanczos_state_words", "bsp_lanczos_work_bytes"] + \
    ["bsp_lanczos_%s%s_%s" % (op, b, t) for op in PIECES for b in ("", "_batched") for t in ("f64", "f32")]
EPS = {np.float64: np.finfo(np.float64).eps, np.float32: float(np.finfo(np.float32).eps)}


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("lanczos", "eig_extremes", "cond2_estimate", "logdet_slq"):
        assert name in S.__all__ and name in S.__doc__ and callable(getattr(S, name)), name
    assert L.STOPS == LR.STOPS and isinstance(L.LanczosRun, type)
    assert "lower bound" in S.cond2_estimate.__doc__ and "kappa_1" in S.cond2_estimate.__doc__
    assert "unbiased" in S.logdet_slq.__doc__


# ---- ABI, plan and refusals ------------------------------------------------------------------------------
def _work_bytes(lib, sol, n, q, kmax):
    need = ctypes.c_int64(-1)
    rc = lib.bsp_lanczos_work_bytes(sol, ctypes.c_int64(n), ctypes.c_int64(q), ctypes.c_int64(kmax), ctypes.byref(need))
    return rc, need.value


def test_state_words_and_work_bytes():
    lib = _lib.load()
    sol = SP.pattern("blocks").solver._h
    words = ctypes.c_int64(0)
    assert lib.bsp_lanczos_state_words(ctypes.byref(words)) == 0 and words.value == 12
    assert lib.bsp_lanczos_state_words(None) != 0
    for n, q, k in ((0, 1, 1), (1, 1, 1), (1024, 3, 18), (1025, 3, 18), (5000, 2, 512)):
        rc, need = _work_bytes(lib, sol, n, q, k)
        # the partials of kmax sums per column, then the kmax projection coefficients per column
        assert rc == 0 and need == 16 * q * k * max(1, (n + 1023) // 1024) + (8 * q * k + 15) // 16 * 16
        assert need % 16 == 0
    base = _work_bytes(lib, sol, 3000, 2, 8)[1]
    assert _work_bytes(lib, sol, 3100, 2, 8)[1] > base          # one more chunk of rows
    assert _work_bytes(lib, sol, 3000, 3, 8)[1] > base
    assert _work_bytes(lib, sol, 3000, 2, 9)[1] > base
    seq = [_work_bytes(lib, sol, n, 2, 8)[1] for n in range(0, 5000, 250)]
    assert seq == sorted(seq)
    for args, msg in (((4, 0, 8), b"q = 0"), ((4, 1, 0), b"kmax = 0"), ((-1, 1, 1), b"n = -1")):
        assert _work_bytes(lib, sol, *args)[0] != 0
        assert msg in lib.bsp_last_error(), (args, lib.bsp_last_error())
    assert _work_bytes(lib, None, 4, 1, 8)[0] != 0
    assert lib.bsp_lanczos_work_bytes(sol, ctypes.c_int64(4), ctypes.c_int64(1), ctypes.c_int64(8), None) != 0


def test_every_entry_refuses_bad_arguments_before_any_launch():
    """fake pointers: a call that got past the checks would fault"""
    lib = _lib.load()
    sol = SP.pattern("blocks").solver._h
    i64, i32, P = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    vec, basis, work, state, coef = P(1 << 20), P(1 << 21), P(1 << 22), P(1 << 23), P(1 << 24)
    mids = {"init": lambda slot, count: (i64(slot), ctypes.c_double(1e-14)),
            "alpha": lambda slot, count: (i64(slot),),
            "update": lambda slot, count: (i64(slot), i64(0), i32(1), coef),
            "project": lambda slot, count: (i64(count),),
            "subtract": lambda slot, count: (i64(count), i32(1), coef),
            "normalize": lambda slot, count: (i64(slot),)}

    def call(piece, sfx="f64", s=sol, n=4, q=1, kmax=8, v=vec, b=basis, stride=4, slots=8, slot=0, count=1, w=work,
             st=state):
        fn = getattr(lib, "bsp_lanczos_%s_%s" % (piece, sfx))
        return fn(s, i64(n), i64(q), i64(kmax), v, b, i64(stride), i64(slots), *mids[piece](slot, count), w, st)

    def refused(msg, *a, **kw):
        assert call(*a, **kw) != 0, (msg, a, kw)
        assert msg in lib.bsp_last_error(), (msg, lib.bsp_last_error(), a, kw)

    for piece in PIECES:
        for sfx in ("f64", "f32"):
            refused(b"solver is NULL", piece, sfx, s=None)
            refused(b"n = -1", piece, sfx, n=-1)
            refused(b"q = 0", piece, sfx, q=0)
            refused(b"kmax = 0", piece, sfx, kmax=0)
            refused(b"workspace pointer is NULL", piece, sfx, w=P(0))
            refused(b"not 16-byte aligned", piece, sfx, w=P((1 << 22) + 8))
            refused(b"state pointer is NULL", piece, sfx, st=P(0))
            refused(b"batch member 0 is NULL", piece, sfx, v=P(0))
            refused(b"basis pointer of batch member 0 is NULL", piece, sfx, b=P(0))
            refused(b"slot stride", piece, sfx, stride=3)
            refused(b"at least one slot", piece, sfx, slots=0)
            if piece in ("project", "subtract"):
                refused(b"count = 9", piece, sfx, count=9)          # outside the basis
                refused(b"count = 0", piece, sfx, count=0)
                refused(b"count = 7", piece, sfx, count=7, kmax=6)  # the work area holds kmax coefficients
            else:
                refused(b"slot 8 is outside the basis of 8 slots", piece, sfx, slot=8)
                refused(b"slot -1 is outside", piece, sfx, slot=-1)
    assert lib.bsp_lanczos_update_f64(sol, i64(4), i64(1), i64(8), vec, basis, i64(4), i64(8), i64(0), i64(8), i32(0),
                                      coef, work, state) != 0
    assert b"previous slot 8 is outside" in lib.bsp_last_error()
    assert lib.bsp_lanczos_update_f64(sol, i64(4), i64(1), i64(8), vec, basis, i64(4), i64(8), i64(0), i64(0), i32(1),
                                      P(0), work, state) != 0
    assert b"coefficient pointer is NULL" in lib.bsp_last_error()
    assert lib.bsp_lanczos_init_f64(sol, i64(4), i64(1), i64(8), vec, basis, i64(4), i64(8), i64(0),
                                    ctypes.c_double(-1.0), work, state) != 0
    assert b"breakdown" in lib.bsp_last_error()
    # the batched forms: an empty batch, NULL pointer arrays, a NULL member
    two = (ctypes.c_void_p * 2)(1 << 20, 0)
    ok2 = (ctypes.c_void_p * 2)(1 << 21, 1 << 25)
    for sfx in ("f64", "f32"):
        fn = getattr(lib, "bsp_lanczos_alpha_batched_" + sfx)
        assert fn(sol, i64(4), i64(1), i64(8), ok2, ok2, i64(4), i64(8), i64(0), work, state, i32(0)) != 0
        assert b"batch is empty" in lib.bsp_last_error()
        assert fn(sol, i64(4), i64(1), i64(8), None, ok2, i64(4), i64(8), i64(0), work, state, i32(2)) != 0
        assert b"w pointers are NULL" in lib.bsp_last_error()
        assert fn(sol, i64(4), i64(1), i64(8), ok2, None, i64(4), i64(8), i64(0), work, state, i32(2)) != 0
        assert b"basis pointers are NULL" in lib.bsp_last_error()
        assert fn(sol, i64(4), i64(1), i64(8), two, ok2, i64(4), i64(8), i64(0), work, state, i32(2)) != 0
        assert b"w pointer of batch member 1 is NULL" in lib.bsp_last_error()
        assert fn(sol, i64(4), i64(1), i64(8), ok2, two, i64(4), i64(8), i64(0), work, state, i32(2)) != 0
        assert b"basis pointer of batch member 1 is NULL" in lib.bsp_last_error()


def test_python_settings_refusals():
    for kw, name in (({"steps": 0}, "steps"), ({"steps": 2.0}, "steps"), ({"steps": True}, "steps"),
                     ({"steps": 513}, "at most 512"), ({"reorth": "selective"}, "reorth"), ({"check_every": 0}, "check_every"),
                     ({"breakdown": -1.0}, "breakdown"), ({"breakdown": float("nan")}, "breakdown")):
        args = {"steps": 8, "reorth": "full", "check_every": None, "breakdown": None}
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            L.check_settings("lanczos", **args)
    L.check_settings("lanczos", 512, None, 1, 0.0)
    assert L.default_breakdown(np.float32) == 64 * EPS[np.float32] == LR.default_breakdown(np.float32)
    z = L.rademacher(40, 3, 7, np.float32)
    assert z.dtype == np.float32 and z.shape == (40, 3) and set(np.unique(z)) == {-1.0, 1.0}
    assert np.array_equal(z, L.rademacher(40, 3, 7, np.float64)) and not np.array_equal(z, L.rademacher(40, 3, 8))


# ---- the restatement against dense numpy -------------------------------------------------------------------
def _dense(n, rows, cols, values):
    A = np.zeros((n, n))
    np.add.at(A, (rows, cols), values)
    return A + np.tril(A, -1).T


def _matrix(name):
    if name == "bs":
        rows, cols, values, A, n = R.bs_case()
        return n, rows, cols, values, A
    rows, cols, values = R.tridiagonal(255)
    return 255, rows, cols, values, _dense(255, rows, cols, values)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name,steps", [("bs", 40), ("tri255", 60)])
def test_basis_is_orthonormal_and_tridiagonalises(name, steps, dt):
    n, rows, cols, values, A = _matrix(name)
    v0 = np.random.default_rng(3).uniform(-1, 1, (n, 2))
    coef, st, V = LR.entries_model(n, rows, cols, values, v0, dt, steps)
    assert V.dtype == dt and (st["steps"] == steps).all(), st
    norm = np.linalg.norm(A, 2)
    for c in range(2):
        Vc = V[:, :, c].astype(np.float64)
        orth = np.abs(Vc @ Vc.T - np.eye(steps)).max()
        T = np.diag(coef[c, 0]) + np.diag(coef[c, 1, :-1], 1) + np.diag(coef[c, 1, :-1], -1)
        tri = np.abs(Vc @ A @ Vc.T - T).max()
        print(name, dt.__name__, "column", c, "max |V V^T - I| =", orth, " max |V A V^T - T| / |A| =", tri / norm)
        assert orth <= (1e-13 if dt is np.float64 else 1e-5)
        # every entry of V A V^T is a sum of n products of rounded numbers, and the columns carry the
        # rounding of `steps` updates: n eps |A| with the factor 8 of the two passes and the three terms
        assert tri <= 8 * n * EPS[dt] * norm
    # without reorthogonalisation the same run loses orthogonality: the bound above tells the two apart
    if name == "bs":
        _, _, V0 = LR.entries_model(n, rows, cols, values, v0, dt, steps, reorth=None)
        lost = np.abs(V0[:, :, 0].astype(np.float64) @ V0[:, :, 0].astype(np.float64).T - np.eye(steps)).max()
        print(name, dt.__name__, "no reorthogonalisation: max |V V^T - I| =", lost)
        assert lost > 1e-3


@pytest.mark.parametrize("dt,bound", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_identity_probes_give_the_exact_logdet(dt, bound):
    rows, cols, values, A, n = R.bs_case()
    coef, st, _ = LR.entries_model(n, rows, cols, values, np.eye(n), dt, n)
    got = sum(L.quadrature(coef[c, 0], coef[c, 1], int(st["steps"][c]), np.log) for c in range(n))
    want = np.linalg.slogdet(A)[1]
    rel = abs(got - want) / abs(want)
    print("identity probes,", dt.__name__, ": logdet", got, "slogdet", want, "relative error", rel)
    assert rel <= bound
    _, ld = np.linalg.slogdet(A)
    coef, st, _ = LR.entries_model(n, rows, cols, values, np.eye(n), dt, n, reorth=None)
    plain = sum(L.quadrature(coef[c, 0], coef[c, 1], int(st["steps"][c]), np.log) for c in range(n))
    print("  without reorthogonalisation: relative error", abs(plain - ld) / abs(ld))


@pytest.mark.parametrize("n,steps", [(255, 40), (255, 120), (1025, 40), (1025, 120)])
def test_ritz_values_lie_within_their_residual_bounds(n, steps):
    rows, cols, values = R.tridiagonal(n)
    lam = 2.5 - 2.0 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1))   # the Toeplitz spectrum (diag 2.5, off -1)
    v0 = np.random.default_rng(n + steps).uniform(-1, 1, (n, 1))
    coef, st, _ = LR.entries_model(n, rows, cols, values, v0, np.float64, steps)
    assert st["steps"][0] == steps and st["stop"][0] == LR.STEP_LIMIT
    theta, tau, bound = L.ritz(coef[0, 0], coef[0, 1], steps)
    assert (np.diff(theta) >= 0).all() and abs(tau.sum() - 1) <= 1e-12
    dist = np.abs(theta[:, None] - lam[None, :]).min(axis=1)
    slack = n * EPS[np.float64] * 4.5                                  # n eps |A|, |A|_2 < 4.5
    assert (dist <= bound + slack).all(), (dist - bound).max()
    assert lam[0] - slack <= theta[0] and theta[-1] <= lam[-1] + slack  # Ritz values lie inside the spectrum


# ---- every stop reason, by a named input -------------------------------------------------------------------
def _diag_model(d, v0, dt, steps, **kw):
    d = np.asarray(d, dtype=np.float64)
    idx = np.arange(len(d))
    return LR.entries_model(len(d), idx, idx, d, v0, dt, steps, **kw)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_stop_invariant_subspace(dt):
    v0 = L.rademacher(16, 1, 1, dt)                # the default start of eig_extremes; its normalisation is exact
    coef, st, V = _diag_model(np.full(16, 2.0), v0, dt, 5)
    assert st["stop"][0] == LR.INVARIANT and st["steps"][0] == 1
    assert abs(coef[0, 0, 0] - 2.0) <= 2.0 * EPS[dt] and not coef[0, :, 1:].any() and not V[1:].any()
    # three distinct eigenvalues: the Krylov space of the ones vector has dimension 3
    d = np.tile([1.0, 2.0, 4.0], 85)
    for reorth in ("full", None):
        coef, st, V = _diag_model(d, np.ones((255, 1)), dt, 10, reorth=reorth)
        assert st["stop"][0] == LR.INVARIANT and st["steps"][0] == 3, (reorth, st)
        theta, tau, bound = L.ritz(coef[0, 0], coef[0, 1], 3)
        np.testing.assert_allclose(theta, [1.0, 2.0, 4.0], rtol=8 * EPS[dt])
        np.testing.assert_allclose(tau, [1 / 3] * 3, rtol=64 * EPS[dt])
        assert not coef[0, :, 3:].any() and not V[3:].any()


def test_stop_zero_start_beside_a_live_column():
    v0 = np.zeros((5, 2))
    v0[:, 1] = [1.0, 2.0, 3.0, 4.0, 5.0]
    coef, st, V = _diag_model([1.0, 2.0, 3.0, 4.0, 5.0], v0, np.float64, 3)
    assert st["stop"].tolist() == [LR.ZERO_START, LR.STEP_LIMIT] and st["steps"].tolist() == [0, 3]
    assert not coef[0].any() and not V[:, :, 0].any() and st["vv"][0] == 0.0
    np.testing.assert_array_equal(LR.record_words(st, 0)[2:7], [0, 0, 0, 0, np.float64(st["thr2"]).view(np.int64)])


def test_stop_non_finite_and_step_limit():
    d = np.array([1.0, 2.0, np.nan, 4.0])
    coef, st, _ = _diag_model(d, np.ones((4, 1)), np.float64, 3)
    assert st["stop"][0] == LR.NON_FINITE and st["steps"][0] == 1 and np.isnan(coef[0, 0, 0])
    v0 = np.ones((4, 1))
    v0[1] = np.inf
    coef, st, _ = _diag_model([1.0, 2.0, 3.0, 4.0], v0, np.float64, 3)
    assert st["stop"][0] == LR.NON_FINITE and st["steps"][0] == 0
    coef, st, _ = _diag_model([1.0, 2.0, 3.0, 4.0], np.ones((4, 1)), np.float64, 2)
    assert st["stop"][0] == LR.STEP_LIMIT and st["steps"][0] == 2 and st["kmax"] == 2
    assert LR.record_words(st, 0)[7] == 2 and not LR.record_words(st, 0)[8:].any()


# ---- post-processing and the order-sensitive pin ----------------------------------------------------------
def test_ritz_and_quadrature_on_a_closed_form_tridiagonal():
    """tridiag(1; 2, 2, 2): theta = 2 - sqrt 2, 2, 2 + sqrt 2 with the eigenvectors (1, -+sqrt 2, 1) / 2 and
    (1, 0, -1) / sqrt 2"""
    alpha, beta = np.array([2.0, 2.0, 2.0, 9.0]), np.array([1.0, 1.0, 0.5, 9.0])
    theta, tau, bound = L.ritz(alpha, beta, 3)
    r2 = np.sqrt(2.0)
    np.testing.assert_allclose(theta, [2 - r2, 2.0, 2 + r2], rtol=1e-14)
    np.testing.assert_allclose(tau, [0.25, 0.5, 0.25], rtol=1e-14)
    np.testing.assert_allclose(bound, 0.5 * np.array([0.5, 1 / r2, 0.5]), rtol=1e-14)   # |beta_2 s_2i|
    # the quadrature is exact for polynomials of degree <= 2 k - 1: e_0^T T^p e_0 = 1, 2, 5, 14
    for p, want in enumerate([1.0, 2.0, 5.0, 14.0]):
        assert abs(L.quadrature(alpha, beta, 3, lambda x: x ** p) - want) <= 1e-13
    assert abs(L.quadrature(alpha, beta, 3, np.log) - np.sum([0.25, 0.5, 0.25] * np.log([2 - r2, 2.0, 2 + r2]))) <= 1e-15
    theta, tau, bound = L.ritz(alpha, beta, 1)
    assert theta.tolist() == [2.0] and tau.tolist() == [1.0] and bound.tolist() == [1.0]
    for bad in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="ritz"):
            L.ritz(alpha, beta, bad)


def test_subtraction_order_of_the_projection_is_ascending():
    """w = 2^54, c_0 v_0 = 1, c_1 v_1 = 2^54: ascending, the 1 is lost against 2^54 (ties to even) and the
    result is 0; descending it would be -1"""
    w = np.array([[2.0 ** 54]])
    vs = np.array([[[1.0]], [[2.0 ** 54]]])
    c = np.array([[1.0], [1.0]])
    assert LR.subtract(w, c, vs, np.float64)[0, 0] == 0.0
    assert LR.subtract(w, c[::-1], vs[::-1], np.float64)[0, 0] == -1.0
    # ... and the products are rounded to the value type before they are subtracted
    w32 = np.array([[1.0]], dtype=np.float32)
    c32 = np.array([[1.0 + 2.0 ** -12]])
    v32 = np.array([[[1.0 + 2.0 ** -12]]], dtype=np.float32)
    want = np.float32(1.0) - np.float32(np.float32(c32[0, 0]) * v32[0, 0, 0])
    assert LR.subtract(w32, c32, v32, np.float32)[0, 0] == want
    assert want != np.float32(1.0 - (1.0 + 2.0 ** -12) ** 2)
    # the projection's sums are dot()'s, whatever their grouping
    rng = np.random.default_rng(0)
    V, x = rng.uniform(-1, 1, (11, 1300, 2)), rng.uniform(-1, 1, (1300, 2))
    np.testing.assert_array_equal(LR.project(V, x), np.stack([R.dot(V[i], x) for i in range(11)]))
