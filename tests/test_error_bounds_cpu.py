"""CPU: the numpy statements of the error bounds (error_bounds_ref.py) against exact
references.  The estimator's restatement must lie in [true / 3, true (1 + 1e-10)] of the 1-norm of the
explicit inverse on every shared matrix, and take each branch of the algorithm where the matrices are built
for it; the residual and maxRatio models must agree with np.longdouble within the bound of a sequential sum.

THE 2x2 CASE.  For A = inv([[1 + e, -1], [-1, 1 + e]]) the algorithm of section 23 measures column 0 of A^-1
in its second pass (z = A^-1 (1, 1) = (e, e) ties, the lowest index wins), which already has the full norm
2 + e, and then stops by "same column".  The alternating vector gives 2 (6 + 3 e) / 6 = 2 + e as well: the two
values tie in exact arithmetic, so which of them `wins` is decided by the last bit.  The test therefore
asserts the stop reason, that the estimate is 1.0000 of the truth, and that the alternating value reaches it
too; it does not assert which side of the tie the rounding falls on.  The alt branch is asserted on
error_bounds_ref.ALT_WINS instead, a 7x7 matrix on which the alternating vector's value wins by 24 %."""
import numpy as np
import pytest

import error_bounds_ref as E
import sym_product_ref as R


@pytest.mark.parametrize("name", E.MATRICES)
def test_estimator_within_three_of_the_truth(name):
    A = E.matrix(name)
    true = E.true_inv_norm1(A)
    est, trace, _ = E.inv_norm1_model(A)
    print("%s: est / true = %.4f, passes %d, stop %s, alt won %s" % (name, est / true, trace["passes"],
                                                                    E.STOPS[trace["stop"]], trace["altWon"]))
    assert true / 3 <= est <= true * (1 + 1e-10)


def test_estimator_scaled():
    A = E.matrix(E.SCALED)
    D = np.sqrt(np.diag(A))
    true = E.true_inv_norm1(A, D)
    est, _, _ = E.inv_norm1_model(A, scale=D)
    assert true / 3 <= est <= true * (1 + 1e-10)
    raw, _, _ = E.inv_norm1_model(A)
    assert raw > 1e10 * est


def test_estimator_branches():
    A = E.matrix("n2")
    true = E.true_inv_norm1(A)
    est, trace, _ = E.inv_norm1_model(A)
    assert E.STOPS[trace["stop"]] == "same column" and trace["passes"] == 2
    assert abs(est / true - 1) < 1e-4
    assert abs(trace["alt"] / true - 1) < 1e-4 and trace["altTie"]
    for name in ("diag7", "identity5"):
        _, trace, fragile = E.inv_norm1_model(E.matrix(name))
        assert E.STOPS[trace["stop"]] == "repeated sign vector" and not fragile, name
    est, trace, _ = E.inv_norm1_model(E.matrix("n1"))
    assert E.STOPS[trace["stop"]] == "order one" and abs(est * 2.5 - 1) < 1e-15
    assert max(E.inv_norm1_model(E.matrix(m))[1]["passes"] for m in E.MATRICES) >= 3
    # the alt branch: the value of the alternating vector strictly wins, in both precisions, nothing fragile
    A = E.matrix(E.ALT_WINS)
    true = E.true_inv_norm1(A)
    for dtype in (np.float64, np.float32):
        est, trace, fragile = E.inv_norm1_model(A, dtype)
        assert trace["altWon"] and est == trace["alt"] and not fragile and not trace["altTie"]
        assert trace["alt"] > 1.2 * trace["main"] and trace["main"] < 0.35 * true
        without, _, _ = E.inv_norm1_model(A, dtype, alt=False)
        assert without == trace["main"]
        est, trace, fragile = E.inv_norm1_model(E.matrix(E.PASS_LIMIT), dtype)
        assert E.STOPS[trace["stop"]] == "pass limit" and trace["passes"] == 5 and not fragile


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["dups", "full", "blocks", "arrow65", "arrow129", "gaps"])
def test_residual_model_against_longdouble(name, dtype):
    c = R.case(name)
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(5)
    v = c["values"].astype(dtype)
    x = rng.uniform(-1, 1, (n, 3)).astype(dtype)
    b = rng.uniform(-1, 1, (n, 3)).astype(dtype)
    r, d = E.residual_model(n, rows, cols, tri, v, x, b, dtype)
    _, t = E.residual_model(n, rows, cols, tri, v, x, None, dtype)
    assert r.dtype == dtype and d.dtype == dtype
    mv = R.mv_model(n, rows, cols, tri, v, x, dtype)
    assert np.array_equal(r, (b - mv).astype(dtype)), "r is not bitwise b - mv"
    Ald = R.dense_ld(n, rows, cols, v)
    absA = R.abs_dense(n, rows, cols, v).astype(np.longdouble)
    bl, xl = b.astype(np.longdouble), x.astype(np.longdouble)
    bound = R.mv_bound(n, rows, cols, tri, v, x, dtype)  # (t_i + 1) eps (|A| |x|)_i
    eps = np.finfo(dtype).eps
    assert np.all(np.abs(r - (bl - Ald @ xl)) <= bound + eps * np.abs(bl - Ald @ xl))
    exact_t = absA @ np.abs(xl)
    assert np.all(np.abs(t - exact_t) <= bound)
    assert np.all(np.abs(d - (exact_t + np.abs(bl))) <= bound + eps * (exact_t + np.abs(bl)))
    # cancelling duplicates do not shrink the scale
    assert np.all(t >= np.abs(mv) * (1 - 200 * eps))


def test_max_ratio_model():
    r = np.array([[0.0, 1.0, np.nan, 1.0, 0.0], [2.0, 1.0, 1.0, np.inf, 0.0]])
    d = np.array([[0.0, 0.0, 1.0, 2.0, 0.0], [4.0, 1.0, 1.0, np.inf, 5.0]])
    got = E.max_ratio(r, d)
    assert got[0] == 0.5 and got[1] == np.inf and np.isnan(got[2]) and np.isnan(got[3]) and got[4] == 0.0
    rng = np.random.default_rng(2)
    r, d = rng.standard_normal((50, 3)), rng.uniform(0.5, 2, (50, 3))
    want = (np.abs(r.astype(np.longdouble)) / d.astype(np.longdouble)).max(0)
    assert np.all(np.abs(E.max_ratio(r, d) - want) <= np.finfo(np.float64).eps * want)
    r32 = r.astype(np.float32)
    assert E.max_ratio(r32, d.astype(np.float32)).dtype == np.float64
    assert np.array_equal(E.col_max(r32), r32.max(0).astype(np.float64))
