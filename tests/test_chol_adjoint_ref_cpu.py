"""CPU: the math and the storage of the factor's reverse mode before any GPU
run.  The numpy restatement of the node recurrence over the selected-inversion plan
(chol_adjoint_ref.recurrence_np) matches the dense torch oracle on every selinv_cases.py skeleton and
on random structures with sparse elimination ranges; the oracle itself matches finite differences."""
import numpy as np
import pytest

from autograd_ref import element_coords
from chol_adjoint_ref import dense_factor, dense_grad, lbar_random, recurrence_np, rel_error
from helpers import solver_random, spd_data
from known_factor import known_factor_data
from selinv_cases import build_case, case_names

TOL = 1e-11  # fp64 recurrence against the fp64 oracle, both on well-conditioned data


def _check(sol, data, seed):
    lbar = lbar_random(sol, seed)
    want = dense_grad(sol, data, lbar)
    got = recurrence_np(sol, dense_factor(sol, data), lbar)
    err = rel_error(got, want)
    assert err < TOL, err
    i, j = element_coords(sol)
    assert (got[i < j] == 0).all()


@pytest.mark.parametrize("name", case_names())
def test_recurrence_matches_oracle_on_selinv_cases(name):
    sol, expect = build_case(name)
    expect(sol._testSelInvPlan())
    _check(sol, known_factor_data(sol, 5, np.float64, rho=0.5).data, 11)


@pytest.mark.parametrize("seed", [3, 8])
def test_recurrence_matches_oracle_on_random_structures(seed):
    sol, _, _ = solver_random(seed, fill=0.037, elim=(0, 60))
    assert len(sol.sparseEliminationRanges()) >= 2
    _check(sol, known_factor_data(sol, seed, np.float64, rho=0.5).data, seed + 1)


def test_oracle_matches_finite_differences():
    sol, _, _ = solver_random(4, size=40, fill=0.1, elim=(0, 20))
    data = spd_data(sol, 2, beta_factor=0.3)
    lbar = lbar_random(sol, 7)
    i, j = element_coords(sol)
    low = i >= j
    grad = dense_grad(sol, data, lbar)
    dirn = np.random.default_rng(1).uniform(-1, 1, sol.dataSize()) * low
    f = lambda d: float(np.dot(lbar[low], dense_factor(sol, d)[low]))
    h = 1e-6
    fd = (f(data + h * dirn) - f(data - h * dirn)) / (2 * h)
    assert abs(fd - np.dot(grad, dirn)) < 1e-7 * max(1.0, abs(fd))


def test_recurrence_ignores_upper_elements_and_needs_every_step():
    """the strictly-upper input elements do not matter; dropping the Schur-update adjoint (step 1)
    is caught"""
    sol, _ = build_case("mixed_owners")
    data = known_factor_data(sol, 2, np.float64, rho=0.5).data
    L = dense_factor(sol, data)
    lbar = lbar_random(sol, 3)
    i, j = element_coords(sol)
    other = lbar.copy()
    other[i < j] = 123.0
    a, b = recurrence_np(sol, L, lbar), recurrence_np(sol, L, other)
    assert np.array_equal(a, b)
    want = dense_grad(sol, data, lbar)
    # a wrong factor (Schur update dropped, i.e. L_RI of a different matrix) changes the result
    assert rel_error(recurrence_np(sol, L * np.where(i > j, 1.01, 1.0), lbar), want) > 1e3 * TOL


def test_entry_points_exist():
    """the C ABI exports the new entry points; Python and autograd expose them"""
    import baspacho_amd as B
    from baspacho_amd import _lib, autograd, sparse
    lib = _lib.load()
    for base in ("bsp_factor_adjoint", "bsp_factor_adjoint_batched", "bsp_pattern_outer", "bsp_pattern_outer_batched"):
        for sfx in ("f64", "f32"):
            assert hasattr(lib, "%s_%s" % (base, sfx))
    assert callable(B.Solver.factorAdjoint) and callable(B.Solver.patternOuter)
    assert all(callable(getattr(autograd, f)) for f in ("cholesky", "solve_l", "solve_lt"))
    assert callable(sparse.sample)
