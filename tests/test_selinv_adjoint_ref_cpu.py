"""CPU: the math and the storage of selected inversion's reverse mode before any
GPU run.  The numpy restatement of the reverse sweep over the selected-inversion plan
(selinv_adjoint_ref.recurrence_np) matches the dense torch oracle on every selinv_cases.py skeleton and
on random structures with sparse elimination ranges; chained with the dense Cholesky adjoint it gives
the projection of -Z S Z; the oracle itself matches finite differences."""
import numpy as np
import pytest

from autograd_ref import element_coords
from chol_adjoint_ref import _Layout, dense_factor, dense_grad
from helpers import solver_random, spd_data
from known_factor import known_factor_data
from selinv_adjoint_ref import dense_lbar, dense_z, grad_random, recurrence_np, rel_error, zsz_projection
from selinv_cases import build_case, case_names

TOL = 1e-11  # fp64 recurrence against the fp64 oracle, both on well-conditioned data


def _check(sol, data, seed):
    L = dense_factor(sol, data)
    _, Z = dense_z(sol, L)
    grad = grad_random(sol, seed)
    coords = element_coords(sol)
    got = recurrence_np(sol, L, Z, grad)
    err = rel_error(got, dense_lbar(sol, L, grad, coords))
    assert err < TOL, err
    i, j = coords
    assert (got[i < j] == 0).all()
    # the chain through the dense Cholesky adjoint against -Z S Z
    err = rel_error(dense_grad(sol, data, got, coords), zsz_projection(sol, L, grad, coords))
    assert err < TOL, err


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
    L = dense_factor(sol, spd_data(sol, 2, beta_factor=0.3))
    grad = grad_random(sol, 7)
    i, j = element_coords(sol)
    lbar = dense_lbar(sol, L, grad)
    dirn = np.random.default_rng(1).uniform(-1, 1, sol.dataSize()) * (i >= j)
    f = lambda l: float(np.dot(grad, dense_z(sol, l)[1]))
    h = 1e-6
    fd = (f(L + h * dirn) - f(L - h * dirn)) / (2 * h)
    assert abs(fd - np.dot(lbar, dirn)) < 1e-7 * max(1.0, abs(fd))


def test_upper_slot_weight_counts_as_its_lower_twin_and_scatter_is_needed():
    """a weight moved from a strictly-upper slot of a diagonal block to its lower twin gives the same
    result to the last bit; dropping the scatter step is caught.  The slots moved are those of the
    first 64 rows of the leaf lump of width 70: both kinds of mirror (inside the node's own block,
    and the node's own-lump rows 64..69 in the columns right of it), and rows that no scatter
    reaches (a slot that a scatter adds to sums its terms in another order after the move)"""
    sol, _ = build_case("mixed_owners")
    data = known_factor_data(sol, 2, np.float64, rho=0.5).data
    L = dense_factor(sol, data)
    _, Z = dense_z(sol, L)
    grad = grad_random(sol, 3)
    i, j = element_coords(sol)
    lay = _Layout(sol)
    off, lw, _, _ = lay.lumps[0]
    assert lw == 70
    e = np.arange(sol.dataSize())
    up = np.nonzero((i < j) & (e >= off) & (e < off + 64 * lw))[0]
    assert (j[up] >= i[up].min() + 64).any() and (j[up] < i[up].min() + 64).any()
    twin = lay.index(j[up], i[up])
    moved = grad.copy()
    moved[twin] += grad[up]
    moved[up] = 0.0
    a, b = recurrence_np(sol, L, Z, grad), recurrence_np(sol, L, Z, moved)
    assert np.array_equal(a, b)
    want = dense_lbar(sol, L, grad)
    assert rel_error(a, want) < TOL
    assert rel_error(recurrence_np(sol, L, Z, grad, scatter=False), want) > 1e3 * TOL


def test_fp32_restatement_stays_near_single_precision():
    """every array of the restatement in float32: the algorithm's own rounding, far below the 1e-4 the
    GPU test allows fp32"""
    sol, _ = build_case("mixed_owners")
    data = known_factor_data(sol, 2, np.float32, rho=0.5).data
    L = dense_factor(sol, data)
    _, Z = dense_z(sol, L)
    grad = grad_random(sol, 3, np.float32)
    got = recurrence_np(sol, L.astype(np.float32), Z.astype(np.float32), grad, dtype=np.float32)
    assert got.dtype == np.float32
    assert rel_error(got, dense_lbar(sol, L, grad)) < 1e-5


def test_entry_points_exist():
    """the C ABI exports the new entry points; Python, autograd and sparse expose them"""
    import baspacho_amd as B
    from baspacho_amd import _lib, autograd, sparse
    lib = _lib.load()
    for base in ("bsp_selected_inverse_adjoint", "bsp_selected_inverse_adjoint_batched"):
        for sfx in ("f64", "f32"):
            assert hasattr(lib, "%s_%s" % (base, sfx))
    assert callable(B.Solver.selectedInverseAdjoint)
    assert callable(autograd.selected_inverse)
    assert callable(sparse.covariance) and callable(sparse.marginal_variances)
