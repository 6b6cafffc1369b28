"""CPU: the gradient extension (logDet / patternGrad / baspacho_amd.autograd) without a GPU.
The eight C entry points must be declared and exported; the reference projection of autograd_ref.py
(dense gradient -> gradient of the stored elements) must agree with central finite differences of
numpy's slogdet and solve; the autograd functions must refuse bad arguments with clear errors."""
import os
import re

import numpy as np
import pytest
import torch

import baspacho_amd as B
from baspacho_amd import _lib
from autograd_ref import element_coords, pattern_grad_ref, project
from helpers import solver_random, spd_data
from selinv_cases import build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bsp_log_det_f64", "bsp_log_det_f32", "bsp_log_det_batched_f64", "bsp_log_det_batched_f32",
           "bsp_pattern_grad_f64", "bsp_pattern_grad_f32", "bsp_pattern_grad_batched_f64",
           "bsp_pattern_grad_batched_f32"]


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name


def _structures():
    return [("random_elim", solver_random(71, size=18, fill=0.12, elim=(0, 8), ranges=[0, 8])[0]),
            ("random", solver_random(72, size=14, fill=0.15)[0]),
            ("small/n3_r170", build_case("small/n3_r170")[0]),
            ("width17", build_case("width17")[0])]


def _dense(sol, d):
    return sol.densify(d, fill_upper_half=True)


def _fd(sol, f, d, idx, h=1e-3):
    out = np.empty(len(idx))
    for t, e in enumerate(idx):
        dp, dm = d.copy(), d.copy()
        dp[e] += h
        dm[e] -= h
        out[t] = (f(dp) - f(dm)) / (2 * h)
    return out


def _sample(sol, rng, count=40):
    i, j = element_coords(sol)
    lower = np.nonzero(i > j)[0]
    diag = np.nonzero(i == j)[0]
    upper = np.nonzero(i < j)[0]
    pick = lambda a: rng.choice(a, size=min(count, len(a)), replace=False) if len(a) else a
    return pick(lower), pick(diag), pick(upper)


@pytest.mark.parametrize("name", [n for n, _ in _structures()])
def test_projection_matches_finite_differences(name):
    sol = dict(_structures())[name]
    rng = np.random.default_rng(5)
    d = spd_data(sol, 11)
    n = sol.order()
    coords = element_coords(sol)
    A = _dense(sol, d)
    Ainv = np.linalg.inv(A)
    b = rng.standard_normal((n, 2))
    w = rng.standard_normal((n, 2))

    # log det: G = A^-1
    f_ld = lambda x: np.linalg.slogdet(_dense(sol, x))[1]
    g_ld = project(sol, Ainv, coords)
    # w . A^-1 b: G = -lam x^T, lam = A^-1 w
    f_sv = lambda x: float(np.sum(w * np.linalg.solve(_dense(sol, x), b)))
    x = np.linalg.solve(A, b)
    lam = np.linalg.solve(A, w)
    g_sv = project(sol, -lam @ x.T, coords)

    lower, diag, upper = _sample(sol, rng)
    for idx in (lower, diag):
        if len(idx) == 0:
            continue
        # (central differences carry the rounding of f / h: bounds relative to the gradient's scale)
        np.testing.assert_allclose(g_ld[idx], _fd(sol, f_ld, d, idx), rtol=1e-4, atol=1e-4 * np.abs(g_ld).max())
        np.testing.assert_allclose(g_sv[idx], _fd(sol, f_sv, d, idx), rtol=1e-4, atol=1e-4 * np.abs(g_sv).max())
    # the strictly-upper elements are not read: perturbing them changes nothing, gradient 0
    if len(upper):
        assert np.all(g_ld[upper] == 0) and np.all(g_sv[upper] == 0)
        assert np.all(_fd(sol, f_ld, d, upper) == 0)
        assert np.all(_fd(sol, f_sv, d, upper) == 0)

    # patternGrad's statement is the same projection: Z = A^-1 on the pattern, U = lam, V = x, -1
    np.testing.assert_allclose(pattern_grad_ref(sol, Z=Ainv[coords], s=1.0, coords=coords), g_ld, rtol=1e-13,
                               atol=1e-15)
    np.testing.assert_allclose(pattern_grad_ref(sol, U=lam, V=x, alpha=-1.0, coords=coords), g_sv,
                               rtol=1e-12, atol=1e-14)


# ---- argument checks of baspacho_amd.autograd (no GPU needed: they come before any device work) ----
@pytest.fixture(scope="module")
def sol():
    return solver_random(73, size=12, fill=0.15)[0]


def _funcs():
    from baspacho_amd import autograd as BA
    return [("solve", lambda s, d, b: BA.solve(s, d, b)), ("logdet", lambda s, d, b: BA.logdet(s, d)),
            ("solve_logdet", lambda s, d, b: BA.solve_logdet(s, d, b))]


@pytest.mark.parametrize("fname", ["solve", "logdet", "solve_logdet"])
def test_rejects_host_tensors(sol, fname):
    fn = dict(_funcs())[fname]
    d = torch.zeros(sol.dataSize(), dtype=torch.float64)
    b = torch.zeros(sol.order(), dtype=torch.float64)
    with pytest.raises(ValueError, match="device memory"):
        fn(sol, d, b)


@pytest.mark.parametrize("fname", ["solve", "logdet", "solve_logdet"])
def test_rejects_wrong_data_size(sol, fname):
    fn = dict(_funcs())[fname]
    with pytest.raises(ValueError, match="dataSize"):
        fn(sol, torch.zeros(sol.dataSize() + 1, dtype=torch.float64), torch.zeros(sol.order(), dtype=torch.float64))
    with pytest.raises(ValueError, match="dataSize"):
        fn(sol, torch.zeros(3, sol.dataSize() - 1, dtype=torch.float64),
           torch.zeros(3, sol.order(), dtype=torch.float64))
    with pytest.raises(TypeError, match="float64 or float32"):
        fn(sol, torch.zeros(sol.dataSize(), dtype=torch.int32), torch.zeros(sol.order(), dtype=torch.int32))


@pytest.mark.parametrize("fname", ["solve", "solve_logdet"])
def test_rejects_bad_rhs(sol, fname):
    fn = dict(_funcs())[fname]
    n, ds = sol.order(), sol.dataSize()
    with pytest.raises(ValueError, match="order"):
        fn(sol, torch.zeros(ds, dtype=torch.float64), torch.zeros(n + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="order"):
        fn(sol, torch.zeros(ds, dtype=torch.float64), torch.zeros(n - 1, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="batch sizes differ"):
        fn(sol, torch.zeros(2, ds, dtype=torch.float64), torch.zeros(3, n, dtype=torch.float64))
    with pytest.raises(TypeError, match="dtype"):
        fn(sol, torch.zeros(ds, dtype=torch.float64), torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match="b must be"):
        fn(sol, torch.zeros(ds, dtype=torch.float64), torch.zeros(1, n, 2, dtype=torch.float64))


def test_import_does_not_pull_torch_into_the_package():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import baspacho_amd; "
            "print('torch' in sys.modules)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "False"
