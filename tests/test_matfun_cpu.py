"""CPU: f(A) v from the Lanczos basis.  The symbols of bsp_krylov_combine_*, every refusal
of the entry (they run on the host), function_coefficients against the closed-form eigen-system of the Toeplitz
tridiagonal, the domain errors, the numpy restatement (matfun_ref.py) against dense U f(Lambda) U^T v at the
bounds of the GPU tests, the restated two-pass route against the restated basis route bit for bit, and the
refusals of the Python layer.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import _lib
from baspacho_amd import lanczos as L
from baspacho_amd import sparse as S
import cg_ref as R
import lanczos_ref as LR
import matfun_ref as MR
import sym_product_ref as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bsp_krylov_combine_%s%s" % (b, t) for b in ("", "batched_") for t in ("f64", "f32")]
FOUR = ["inv_sqrt", "sqrt", "inv", "log"]


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("apply_function", "sample_lanczos", "sample_cov_lanczos"):
        assert name in S.__all__ and name in S.__doc__ and callable(getattr(S, name)), name
    assert callable(L.function_coefficients) and callable(L.apply_function) and callable(L.LanczosRun.combine)
    assert "not a bound" in S.apply_function.__doc__ and "cond2_estimate" in S.apply_function.__doc__


def test_every_refusal_runs_on_the_host():
    """fake pointers: a call that got past the checks would fault"""
    lib = _lib.load()
    sol = SP.pattern("blocks").solver._h
    i64, i32, P = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    basis, y, limit, out = P(1 << 20), P(1 << 21), P(1 << 22), P(1 << 23)

    def call(sfx="f64", s=sol, n=4, q=2, nf=1, b=basis, stride=8, slots=8, slot=0, count=8, first=0, yy=y, ldy=8,
             lim=limit, o=out, ostride=8, acc=0, batch=None):
        fn = getattr(lib, "bsp_krylov_combine_%s%s" % ("" if batch is None else "batched_", sfx))
        tail = () if batch is None else (i32(batch),)
        return fn(s, i64(n), i64(q), i32(nf), b, i64(stride), i64(slots), i64(slot), i64(count), i64(first), yy, i64(ldy),
                  lim, o, i64(ostride), i32(acc), *tail)

    def refused(msg, **kw):
        assert call(**kw) != 0, (msg, kw)
        assert msg in lib.bsp_last_error(), (msg, lib.bsp_last_error(), kw)

    for sfx in ("f64", "f32"):
        refused(b"solver is NULL", sfx=sfx, s=None)
        refused(b"n = -1", sfx=sfx, n=-1)
        refused(b"q = 0", sfx=sfx, q=0)
        refused(b"nf = 0", sfx=sfx, nf=0)
        refused(b"nf = 5", sfx=sfx, nf=5)
        refused(b"count = 0", sfx=sfx, count=0)
        refused(b"first = -1", sfx=sfx, first=-1)
        refused(b"slot = -1", sfx=sfx, slot=-1)
        refused(b"outside the basis of 8 slots", sfx=sfx, slot=1)            # slot + count = 9
        refused(b"outside the basis of 8 slots", sfx=sfx, count=9, ldy=9)
        refused(b"outside the basis of 0 slots", sfx=sfx, slots=0)
        refused(b"slot stride 7", sfx=sfx, stride=7)
        refused(b"output stride 7", sfx=sfx, ostride=7)
        refused(b"ldy = 7", sfx=sfx, ldy=7)
        refused(b"coefficient pointer is NULL", sfx=sfx, yy=P(0))
        refused(b"limit pointer is NULL", sfx=sfx, lim=P(0))
        refused(b"basis pointer of batch member 0 is NULL", sfx=sfx, b=P(0))
        refused(b"output pointer of batch member 0 is NULL", sfx=sfx, o=P(0))
        # the batched form: an empty batch, NULL pointer arrays, a NULL member
        ok2 = (ctypes.c_void_p * 2)(1 << 20, 1 << 25)
        two = (ctypes.c_void_p * 2)(1 << 20, 0)
        refused(b"batch is empty", sfx=sfx, b=ok2, o=ok2, batch=0)
        refused(b"basis pointers are NULL", sfx=sfx, b=None, o=ok2, batch=2)
        refused(b"output pointers are NULL", sfx=sfx, b=ok2, o=None, batch=2)
        refused(b"basis pointer of batch member 1 is NULL", sfx=sfx, b=two, o=ok2, batch=2)
        refused(b"output pointer of batch member 1 is NULL", sfx=sfx, b=ok2, o=two, batch=2)
        # n == 0 succeeds without a launch (and without a device)
        assert call(sfx=sfx, n=0, stride=0, ostride=0) == 0, lib.bsp_last_error()
        assert call(sfx=sfx, n=0, stride=0, ostride=0, b=ok2, o=ok2, batch=2) == 0, lib.bsp_last_error()


# ---- the host coefficients -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_function_coefficients_on_the_closed_form_tridiagonal(k):
    """T = tridiag(-1; 2.5) of cg_ref.tridiagonal: theta_j = 2.5 - 2 cos(j pi / (k + 1)) with the eigenvectors
    s_ij = sqrt(2 / (k + 1)) sin(i j pi / (k + 1)), i, j = 1 .. k"""
    rows, cols, values = R.tridiagonal(max(k, 2))
    alpha = np.full(k + 1, values[0])
    beta = np.full(k + 1, values[-1])            # (the entry behind the k-th is not part of T_k)
    beta[k - 1] = 77.0
    j = np.arange(1, k + 1)
    theta = 2.5 - 2.0 * np.cos(j * np.pi / (k + 1))
    s = np.sqrt(2.0 / (k + 1)) * np.sin(np.outer(j, j) * np.pi / (k + 1))
    fs = {"sqrt": np.sqrt, "inv_sqrt": lambda t: 1 / np.sqrt(t), "inv": lambda t: 1 / t, "log": np.log,
          ("exp", 0.5): lambda t: np.exp(-0.5 * t), ("pow", 3): lambda t: t ** 3, ("pow", -1.5): lambda t: t ** -1.5}
    for f, fn in fs.items():
        want = 3.0 * (s @ (fn(theta) * s[0]))
        got = L.function_coefficients(alpha, beta, k, f, 3.0)
        assert got.shape == (k,) and np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (f, k)
        again = L.function_coefficients(alpha, beta, k, fn, 3.0)      # the same function as a callable
        assert np.abs(again - want).max() <= 1e-13 * np.abs(want).max(), (f, k)
    # dense eigh of the same matrix
    T = np.diag(alpha[:k]) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    lam, U = np.linalg.eigh(T)
    want = 2.0 * (U @ (np.log(lam) * U[0]))
    assert np.abs(L.function_coefficients(alpha, beta, k, "log", 2.0) - want).max() <= 1e-14 * max(np.abs(want).max(), 1)
    # the identity as a callable: T e_1
    got = L.function_coefficients(alpha, beta, k, lambda t: t, 1.0)
    assert np.abs(got - T[:, 0]).max() <= 1e-14 * 2.5


def test_function_coefficients_refusals_and_domain():
    alpha, beta = np.array([1.0, -2.0, 3.0]), np.array([0.0, 0.0, 0.0])     # Ritz values -2, 1, 3
    for f, word in (("inv_sqrt", "<= 0"), ("inv", "<= 0"), ("log", "<= 0"), (("pow", 0.5), "<= 0"), ("sqrt", "< 0")):
        with pytest.raises(B.FactorizationError, match=r"Ritz value -2 of column 4 of batch member 1 is %s" % word) as e:
            L.function_coefficients(alpha, beta, 3, f, 1.0, column=4, member=1)
        assert e.value.status == {"column": 4, "member": 1, "theta_min": -2.0}
    with pytest.raises(B.FactorizationError, match="Ritz value 0 of column 0 is <= 0"):
        L.function_coefficients([0.0], [0.0], 1, "inv", 1.0, column=0)
    assert L.function_coefficients([0.0], [0.0], 1, "sqrt", 1.0).tolist() == [0.0]           # 0 is in sqrt's domain
    np.testing.assert_allclose(L.function_coefficients(alpha, beta, 3, ("pow", 2), 1.0), [1.0, 0.0, 0.0], atol=1e-15)
    np.testing.assert_allclose(L.function_coefficients(alpha, beta, 3, ("exp", 1.0), 2.0), [2 * np.exp(-1.0), 0, 0], atol=1e-15)
    for bad in (lambda t: t[:-1], lambda t: np.full(t.shape, np.nan), lambda t: np.log(t), lambda t: "x"):
        with pytest.raises(ValueError, match="finite array"):
            L.function_coefficients(alpha, beta, 3, bad, 1.0)
    for f in ("cos", ("exp",), ("exp", "t"), ("pow", float("inf")), ("sin", 1.0), 3, None, ("exp", True)):
        with pytest.raises(ValueError, match="f must be"):
            L.function_coefficients(alpha, beta, 3, f, 1.0)
    for k in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="function_coefficients"):
            L.function_coefficients(alpha, beta, k, "inv", 1.0)


# ---- the combine, restated -----------------------------------------------------------------------------------
def test_combine_order_rounding_limits_and_accumulate():
    # ascending: 2^54 + 1 - 2^54 is 0 (the 1 is lost), descending it would be 1
    vs = np.array([[[2.0 ** 54]], [[1.0]], [[-2.0 ** 54]]])
    y = np.ones((1, 1, 3))
    assert MR.combine(vs, y, [3], np.float64)[0, 0, 0] == 0.0
    assert MR.combine(vs[::-1], y, [3], np.float64)[0, 0, 0] == 0.0 and MR.combine(vs[[1, 0, 2]], y, [3], np.float64)[0, 0, 0] == 0.0
    assert MR.combine(vs[[0, 2, 1]], y, [3], np.float64)[0, 0, 0] == 1.0
    # the coefficient is rounded to the value type, then the product
    c = 1.0 + 2.0 ** -24 + 2.0 ** -40          # float32(c) = 1 + 2^-23; 3 c is 0.75 ulp above 3, 3 float32(c) 1.5 ulp
    got = MR.combine(np.array([[[3.0]]], dtype=np.float32), np.array([[[c]]]), [1], np.float32)[0, 0, 0]
    assert got == np.float32(np.float32(c) * np.float32(3.0)) == np.float32(3.0 + 2.0 ** -21) and got != np.float32(c * 3.0)
    # limits per column, NaN beyond them, several outputs, and a chain of calls against one call
    rng = np.random.default_rng(1)
    for dt in (np.float64, np.float32):
        vs = rng.uniform(-1, 1, (9, 5, 3)).astype(dt)
        y = rng.uniform(-1, 1, (3, 2, 9))
        limit = np.array([0, 4, 11])
        first = 2
        for i in range(9):
            vs[i][:, first + i >= limit] = np.nan
        whole = MR.combine(vs, y, limit, dt, first=first)
        assert whole.dtype == dt and np.isfinite(whole).all() and not whole[:, :, 0].any() and not np.signbit(whole[:, :, 0]).any()
        chain = None
        for a, b in ((0, 1), (1, 4), (4, 9)):
            chain = MR.combine(vs[a:b], y[:, :, a:b], limit, dt, out=chain, first=first + a)
        assert chain.tobytes() == whole.tobytes()
        for f in range(2):
            assert MR.combine(vs, y[:, f:f + 1], limit, dt, first=first).tobytes() == whole[f:f + 1].tobytes()
        seed = rng.uniform(-1, 1, (2, 5, 3)).astype(dt)
        acc = MR.combine(vs, y, limit, dt, out=seed, first=first)
        assert acc[:, :, 0].tobytes() == seed[:, :, 0].tobytes() and acc[:, :, 1].tobytes() != seed[:, :, 1].tobytes()


# ---- the restatement against dense numpy ---------------------------------------------------------------------
def _dense(n, rows, cols, values):
    A = np.zeros((n, n))
    np.add.at(A, (rows, cols), values)
    return A + np.tril(A, -1).T


def _model(n, rows, cols, values, v0, dt, fs, steps, **kw):
    prod = R.Product(n, rows, cols)
    return MR.apply_function_model(n, lambda v: prod.mv(values, v, dt), v0, dt, fs, steps, **kw)


@pytest.mark.parametrize("dt,bound", [(np.float64, 1e-11), (np.float32, 1e-3)])
def test_restatement_is_exact_at_n_steps(dt, bound):
    rows, cols, values, A, n = R.bs_case()
    v0 = np.random.default_rng(21).uniform(-1, 1, (n, 2)).astype(dt)
    out, info = _model(n, rows, cols, values, v0, dt, FOUR, n)
    assert out.dtype == dt and (info["steps"] == n).all()
    Ad = _dense(n, rows, cols, values.astype(dt).astype(np.float64))
    for j, f in enumerate(FOUR):
        err = MR.rel_err(out[j], MR.dense_function(Ad, f, v0))
        print("bs_case, %d steps, full, %s, %s: relative error %s (bound %g), change %s"
              % (n, dt.__name__, f, err, bound, info["change"][j]))
        assert (err <= bound).all(), (f, err)
    if dt is np.float64:
        out, info = _model(n, rows, cols, values, v0, dt, [("exp", 0.5)], 24)
        err = MR.rel_err(out[0], MR.dense_function(Ad, ("exp", 0.5), v0))
        print("bs_case, 24 steps, full, float64, exp(-A / 2): relative error %s (bound 1e-12)" % err)
        assert (err <= 1e-12).all(), err
        out, info = _model(n, rows, cols, values, v0, dt, ["inv_sqrt"], 32)
        err = MR.rel_err(out[0], MR.dense_function(Ad, "inv_sqrt", v0))
        print("bs_case, 32 of 40 steps, inv_sqrt: relative error %s, change %s: error / change %s"
              % (err, info["change"][0], err / info["change"][0]))
        assert (err > 1e-4).all()          # kappa_2 = 1e3: not converged before the Krylov space is exhausted


@pytest.mark.parametrize("dt,bound", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_restated_two_pass_is_the_basis_route_bit_for_bit(dt, bound):
    n = 1500
    rows, cols, values = R.tridiagonal(n)
    v0 = np.random.default_rng(22).uniform(-1, 1, (n, 2)).astype(dt)
    basis, info = _model(n, rows, cols, values, v0, dt, FOUR, 48, reorth=None)
    twice, info2 = _model(n, rows, cols, values, v0, dt, FOUR, 48, reorth=None, memory="two_pass")
    assert basis.tobytes() == twice.tobytes() and info["coef"].tobytes() == info2["coef"].tobytes()
    Ad = _dense(n, rows, cols, values.astype(dt).astype(np.float64))
    for j, f in enumerate(FOUR):
        err = MR.rel_err(basis[j], MR.dense_function(Ad, f, v0))
        print("tridiagonal(1500), 48 steps, reorth None, %s, %s: relative error %s (bound %g)" % (dt.__name__, f, err, bound))
        assert (err <= bound).all(), (f, err)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_restated_two_pass_with_stopped_zero_and_nan_columns(dt):
    """the order-255 diagonal that repeats 1, 2, 4, with 45 distinct values behind it: the ones vector of the first
    block spans an invariant subspace of dimension 3, a random vector does not"""
    d = np.concatenate([np.tile([1.0, 2.0, 4.0], 85), 5.0 + np.arange(45)])
    n = len(d)
    v0 = np.random.default_rng(23).uniform(-1, 1, (n, 4))
    v0[:, 0] = 0.0
    v0[:255, 0] = 1.0
    v0[:, 1] = 0.0
    v0[7, 3] = np.inf
    op = lambda v: (d[:, None].astype(dt) * v).astype(dt)
    basis, info = MR.apply_function_model(n, op, v0, dt, ["inv_sqrt", "log"], 10, reorth=None)
    twice, _ = MR.apply_function_model(n, op, v0, dt, ["inv_sqrt", "log"], 10, reorth=None, memory="two_pass")
    assert info["steps"].tolist() == [3, 0, 10, 0] and info["stop"].tolist() == [LR.INVARIANT, LR.ZERO_START,
                                                                                LR.STEP_LIMIT, LR.NON_FINITE]
    assert basis.tobytes() == twice.tobytes()
    assert not basis[:, :, 1].any() and not np.signbit(basis[:, :, 1]).any() and np.isnan(basis[:, :, 3]).all()
    eps = float(np.finfo(dt).eps)
    np.testing.assert_allclose(basis[0][:255, 0], 1 / np.sqrt(d[:255]), rtol=64 * eps)     # exact in the invariant subspace
    np.testing.assert_allclose(basis[1][:255, 0], np.log(d[:255]), rtol=0, atol=64 * eps)
    assert not basis[:, 255:, 0].any()


def test_restated_identity_probes():
    rows, cols, values, A, n = R.bs_case()
    out, _ = _model(n, rows, cols, values, np.eye(n), np.float64, ["inv_sqrt"], n)
    X = out[0]
    inv = np.linalg.inv(A)
    e1 = np.abs(X @ X.T - inv).max() / np.abs(inv).max()
    e2 = np.abs(X - X.T).max() / np.abs(X).max()
    print("identity probes: max |X X^T - inv(A)| / max |inv(A)| = %g, max |X - X^T| / max |X| = %g (bounds 1e-11)" % (e1, e2))
    assert e1 <= 1e-11 and e2 <= 1e-11


# ---- the Python layer ------------------------------------------------------------------------------------------
def test_python_refusals():
    with pytest.raises(ValueError, match="needs reorth=None"):
        L.apply_function(None, None, None, ["inv"], 8, "full", "two_pass")
    with pytest.raises(ValueError, match="memory must be"):
        L.apply_function(None, None, None, ["inv"], 8, None, "ring")
    with pytest.raises(ValueError, match="between 1 and 4"):
        L.apply_function(None, None, None, ["inv"] * 5, 8)
    with pytest.raises(ValueError, match="between 1 and 4"):
        L.apply_function(None, None, None, [], 8)
    with pytest.raises(ValueError, match="f must be"):
        L.apply_function(None, None, None, ["cos"], 8)
    with pytest.raises(ValueError, match="steps"):
        L.apply_function(None, None, None, ["inv"], 0)
    pat = SP.pattern("blocks")
    values = torch.ones(pat.nnz, dtype=torch.float64, requires_grad=True)
    for fn, args in ((S.apply_function, ("inv",)), (S.sample_lanczos, ()), (S.sample_cov_lanczos, ())):
        with pytest.raises(ValueError, match="gradients in values .* are not provided"):
            fn(pat, values, torch.ones(pat.n, dtype=torch.float64), *args)
