"""CPU: the reference and the metric of the selected-inversion tests (selinv_ref.py) check what they
claim.  Errors planted in an exact Z are caught in correlation units where the former max-normalised
metric lets them pass; the oracle's columns of A^-1 agree with the dense inverse."""
import numpy as np
import pytest

from helpers import solver_random, spd_data
from selinv_ref import corr_error, corr_error_columns, dense_reference, max_normalised_error, \
    oracle_columns, pattern_of, stored_entries, SkelBuilder

TOL64 = 2.5e-14     # fp64 bound of test_selinv_gpu.py / test_selinv_edges_gpu.py
OLD_TOL64 = 1e-10   # the former max-normalised bound


def _scaled_problem():
    """A = D A0 D with D = 10^1.5 on the rows of lumps 0 and 1: their variances are 1e-3 of the
    others', so sqrt(Z_ii Z_jj) ~ 1e-3 max|Z| on their blocks (diagonal ones and the one between)"""
    b = SkelBuilder()
    l0, l1, l2 = b.lump([2, 3]), b.lump([4]), b.lump([3, 3])
    b.couple(l0, l1, l2)
    sol = b.solver()
    A0 = sol.densify(spd_data(sol, 9), fill_upper_half=True)
    d = np.ones(sol.order())
    n_small = int(sol.skel()["lumpStart"][2])
    d[:n_small] = 10 ** 1.5
    Z = np.linalg.inv(d[:, None] * A0 * d[None, :])
    return sol, 0.5 * (Z + Z.T), n_small


@pytest.mark.parametrize("where", ["off_diagonal_block", "upper_triangle_of_diagonal_block"])
def test_planted_error_fails_new_metric_passes_old(where):
    sol, Z, n_small = _scaled_problem()
    rows, cols, lump = stored_entries(sol)
    exact = pattern_of(sol, Z)
    assert corr_error(sol, exact, Z).value < 1e-14
    dz = np.diag(Z)
    scale = np.sqrt(dz[rows] * dz[cols]) / np.abs(Z).max()
    ls = sol.skel()["lumpStart"]
    lump_of_row = np.searchsorted(ls, rows, side="right") - 1
    if where == "off_diagonal_block":
        cand = lump_of_row != lump          # a block below the diagonal block of its lump
    else:
        cand = rows < cols                  # strictly upper triangle of a diagonal block
    cand &= (rows < n_small) & (cols < n_small) & (scale > 3e-4) & (scale < 3e-3)
    idx = np.nonzero(cand)[0]
    assert len(idx), "no stored entry of the intended kind"
    i = idx[0]
    got = exact.copy()
    got[i] += 5e-11 * np.abs(Z).max()
    assert max_normalised_error(sol, got, Z) < OLD_TOL64     # the former metric misses it
    e = corr_error(sol, got, Z)
    assert e.value > 10 * TOL64, e                           # this one does not
    assert "(%d, %d)" % (rows[i], cols[i]) in e.where and "lump %d" % lump[i] in e.where


def test_metric_reports_non_finite():
    sol, Z, _ = _scaled_problem()
    got = pattern_of(sol, Z)
    got[7] = np.nan
    assert corr_error(sol, got, Z).value == np.inf


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dense_reference_and_oracle_columns(dtype):
    """inv() of the rounded input is an accurate inverse; the oracle's columns match it"""
    sol, ps, _ = solver_random(59, fill=0.05, elim=(0, 40))
    data = spd_data(sol, 4, dtype=dtype)
    A, X, res = dense_reference(sol, data)
    assert res < 1e-13
    spans = [0, 7, sol.numSpans() - 1]
    idx, cols = oracle_columns(sol, data.astype(np.float64), spans)
    assert np.abs(cols - X[:, idx]).max() / np.abs(X).max() < 1e-13
    e = corr_error_columns(sol, pattern_of(sol, X), idx, cols)
    assert e.value < 1e-13, e
