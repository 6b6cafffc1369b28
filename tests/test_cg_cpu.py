"""CPU: the numpy restatement of the device-resident conjugate gradient (cg_ref.py)
against numpy.linalg.solve and the textbook step bound, every stop reason reached by a named input, the host
plan of the built-in preconditioners against its restatement, and the argument refusals.  No GPU."""
import os
import re

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import _lib, pcg
from baspacho_amd import cg as CG
from baspacho_amd import sparse as S
from assembly_ref import dense_user, duplicated
import cg_ref as R
import sym_product_ref as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = ("init", "alpha", "update", "precond", "direction", "precond_build")
SYMBOLS = ["bsp_cg_state_words", "bsp_cg_work_bytes", "bsp_cg_precond_info", "bsp_cg_precond_table"] + \
    ["bsp_cg_%s%s_%s" % (op, b, t) for op in PIECES for b in ("", "_batched") for t in ("f64", "f32")]

SIZES, TOL, bs_case = R.BS_SIZES, R.TOL, R.bs_case


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
    assert "solve_cg" in S.__all__ and "solve_cg" in S.__doc__ and callable(S.solve_cg)
    assert isinstance(pcg.DevicePCG, type) and CG.STOPS == R.STOPS


# ---- the pieces of the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1024, 1025, 4097, 256 * 1024 + 1])
def test_ordered_sum_is_a_sum(n):
    rng = np.random.default_rng(n)
    v = rng.uniform(-1, 1, (n, 2))
    got = R.ordered_sum(v)
    want = np.array([float(np.sum(v[:, j].astype(np.longdouble))) for j in range(2)])
    assert np.all(np.abs(got - want) <= 64 * np.finfo(np.float64).eps * np.abs(v).sum(0) + 0.0)
    # integers sum exactly, whatever the order: every row is taken exactly once
    k = rng.integers(-1000, 1000, (n, 2)).astype(np.float64)
    np.testing.assert_array_equal(R.ordered_sum(k), k.sum(0))


def test_ordered_sum_order_is_the_stated_one():
    """2^53 at row 0, then 1.0 at the rows thread 0 takes next: added one by one each is lost; added to each
    other first they are not.  Pins the per-thread row order and the fold"""
    v = np.zeros((1025, 1))
    v[0] = 2.0 ** 53
    v[[256, 512, 768]] = 1.0            # thread 0's later rows: lost one by one
    assert R.ordered_sum(v)[0] == 2.0 ** 53
    v[[256, 512, 768]] = 0.0
    v[[128, 64]] = 1.0                  # threads 128 and 64: folded into thread 0 at s = 128 and s = 64, lost
    assert R.ordered_sum(v)[0] == 2.0 ** 53
    v[[128, 64]] = 0.0
    v[[192, 64]] = 1.0                  # thread 192 folds into 64 first (s = 128): 2.0 survives
    assert R.ordered_sum(v)[0] == 2.0 ** 53 + 2.0
    v[[192, 64]] = 0.0
    v[1024] = 1.0                       # the second chunk's partial is merged after the fold of the first
    assert R.ordered_sum(v)[0] == 2.0 ** 53


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["dups", "full", "blocks", "arrow65", "gaps"])
def test_vectorised_product_is_the_stated_fold(name, dt):
    c = SP.case(name)
    x = np.random.default_rng(3).uniform(-1, 1, (c["n"], 3))
    got = R.Product(c["n"], c["rows"], c["cols"], c["triangle"]).mv(c["values"], x, dt)
    want = SP.mv_model(c["n"], c["rows"], c["cols"], c["triangle"], c["values"], x, dt)
    assert got.dtype == dt and got.tobytes() == want.tobytes()


# ---- the iteration against numpy --------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
def test_grid_laplacian_against_numpy(precond):
    n, rows, cols, values = SP.grid_entries(12, 0.1)
    A = dense_user(n, rows, cols, values)
    kappa = np.linalg.cond(A)
    b = np.random.default_rng(1).uniform(-1, 1, (n, 2))
    x, st, status = R.entries_model(n, rows, cols, values, b, np.float64, precond, tol=TOL, max_steps=200)
    assert (st["stop"] == R.CONVERGED).all()
    want = np.linalg.solve(A, b)
    # |x - x*| / |x*| <= kappa |r| / |b|, the recurrence residual within tol (drift is far below it here)
    err = np.linalg.norm(x - want, axis=0) / np.linalg.norm(want, axis=0)
    assert (err <= 2 * kappa * TOL).all(), err
    true_res = np.linalg.norm(b - A @ x, axis=0) / np.linalg.norm(b, axis=0)
    assert (true_res <= 2 * TOL).all()
    # the diagonal is constant: Jacobi scales the iteration without changing its steps by more than rounding
    assert (st["iterations"] <= R.cg_bound(kappa, TOL)).all(), (st["iterations"], R.cg_bound(kappa, TOL))
    if precond is not None:
        np.testing.assert_array_equal(status, [-1, 0])


@pytest.mark.parametrize("dt,tol", [(np.float64, TOL), (np.float32, 1e-4)])
@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
def test_block_sparse_against_numpy(precond, dt, tol):
    rows, cols, values, A, n = bs_case()
    kappa = np.linalg.cond(A)
    assert kappa <= 1e3 * (1 + 1e-9)
    b = np.random.default_rng(2).uniform(-1, 1, (n, 3))
    x, st, status = R.entries_model(n, rows, cols, values, b, dt, precond, param_sizes=SIZES, tol=tol, max_steps=400)
    assert x.dtype == dt and (st["stop"] == R.CONVERGED).all(), st
    want = np.linalg.solve(A, b)
    err = np.linalg.norm(x - want, axis=0) / np.linalg.norm(want, axis=0)
    assert (err <= 2 * kappa * tol).all(), err
    if precond is None and dt == np.float64:
        assert (st["iterations"] <= R.cg_bound(kappa, tol)).all(), (st["iterations"], R.cg_bound(kappa, tol))
    rel = np.sqrt(st["rr"] / st["bb"])
    assert (rel <= tol).all()


def test_preconditioner_restatement_inverts_the_blocks():
    rows, cols, values, A, n = bs_case()
    plan = R.precond_plan(n, rows, cols, "lower", SIZES)
    minv, off, status = R.build_block(plan, values, np.float64)
    np.testing.assert_array_equal(status, [-1, 0])
    bs = plan[0]
    for b, w in enumerate(SIZES):
        blk = A[bs[b]:bs[b + 1], bs[b]:bs[b + 1]]
        got = minv[off[b]:off[b + 1]].reshape(w, w)
        np.testing.assert_allclose(got @ blk, np.eye(w), atol=1e-10)
        assert np.array_equal(got, got.T)
    inv, status = R.build_jacobi(R.precond_plan(n, rows, cols, "lower"), values, np.float32)
    assert inv.dtype == np.float32
    np.testing.assert_array_equal(inv, (1.0 / np.diag(A).astype(np.float32).astype(np.float64)).astype(np.float32))


# ---- every stop reason, by a named input --------------------------------------------------------------
def _dense_model(A, b, dt=np.float64, apply_m=None, **kw):
    A = np.asarray(A, dtype=np.float64)
    i, j = np.nonzero(np.tril(A) != 0)
    prod = R.Product(A.shape[0], i, j)
    v = A[i, j]
    return R.cg_model(A.shape[0], lambda p: prod.mv(v, p, dt), b, dt, apply_m, **kw)


def test_stop_breakdown():
    x, st = _dense_model(np.diag([1.0, -1.0]), np.array([1.0, 1.0]), max_steps=10)
    assert st["stop"][0] == R.BREAKDOWN and st["iterations"][0] == 0 and st["pAp"][0] == 0.0
    np.testing.assert_array_equal(x[:, 0], [0.0, 0.0])
    # ... and through a preconditioner that is not positive definite: r.z = 1 - 1
    x, st = _dense_model(np.eye(2), np.array([1.0, 1.0]), apply_m=lambda r: r * np.array([[1.0], [-1.0]]), max_steps=10)
    assert st["stop"][0] == R.BREAKDOWN and st["iterations"][0] == 0 and st["rz"][0] == 0.0


def test_stop_zero_rhs_beside_a_live_column():
    A = SP.dense_ld(4, *R.tridiagonal(4)).astype(np.float64)
    b = np.zeros((4, 2))
    b[:, 1] = [1.0, 2.0, 3.0, 4.0]
    x, st = _dense_model(A, b, max_steps=10, x0=np.ones((4, 2)))
    assert st["stop"][0] == R.ZERO_RHS and st["iterations"][0] == 0 and st["bb"][0] == 0.0
    assert not x[:, 0].any() and np.isfinite(x).all()
    assert st["stop"][1] == R.CONVERGED
    np.testing.assert_allclose(A @ x[:, 1], b[:, 1], rtol=1e-9)


def test_stop_eigenvector_after_one_step_beside_a_slow_column():
    n = 64
    rows, cols, values = R.tridiagonal(n)
    A = dense_user(n, rows, cols, values)
    k = np.arange(1, n + 1)
    v = np.sin(np.pi * 3 * k / (n + 1))            # an eigenvector of the Toeplitz tridiagonal matrix
    b = np.stack([v, np.random.default_rng(0).uniform(-1, 1, n)], axis=1)
    x1, st1, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=1e-8, max_steps=1)
    x, st, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=1e-8, max_steps=40)
    assert st["stop"][0] == R.CONVERGED and st["iterations"][0] == 1
    assert st["iterations"][1] > 10
    # frozen: the eigenvector column is bitwise what it was at its stop, while its neighbour went on
    assert x[:, 0].tobytes() == x1[:, 0].tobytes()
    for key in ("rz", "pAp", "rr", "bb", "alpha", "beta"):
        assert st[key][0] == st1[key][0]
    assert st1["stop"][1] == R.STEP_LIMIT and st1["iterations"][1] == 1


def test_stop_non_finite_and_step_limit():
    n, rows, cols, values = SP.grid_entries(5, 0.1)
    b = np.ones((n, 2))
    bad = values.copy()
    bad[3] = np.nan
    x, st, _ = R.entries_model(n, rows, cols, bad, b, np.float64, None, tol=TOL, max_steps=10)
    assert (st["stop"] == R.NON_FINITE).all() and (st["iterations"] == 0).all()
    b[0, 1] = np.inf
    x, st, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=TOL, max_steps=10)
    assert st["stop"][1] == R.NON_FINITE and st["stop"][0] == R.CONVERGED
    b = np.random.default_rng(4).uniform(-1, 1, (n, 1))
    x, st, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=1e-300, max_steps=3)
    assert st["stop"][0] == R.STEP_LIMIT and st["iterations"][0] == 3
    x0, st0, _ = R.entries_model(n, rows, cols, values, b, np.float64, None, tol=TOL, max_steps=0)
    assert st0["stop"][0] == R.STEP_LIMIT and st0["iterations"][0] == 0 and not x0.any()


def test_bad_block_is_reported_not_propagated():
    rows, cols, values, A, n = bs_case()
    bs = np.concatenate([[0], np.cumsum(SIZES)])
    v = values.copy()
    k = int(np.nonzero((rows == bs[2] + 4) & (cols == bs[2] + 4))[0][0])
    v[k] = -5.0                                    # scalar 4 of param 2: its pivot fails at or before it
    plan = R.precond_plan(n, rows, cols, "lower", SIZES)
    minv, off, status = R.build_block(plan, v, np.float64)
    assert status[1] == 1 and bs[2] <= status[0] <= bs[2] + 4
    assert not minv[off[2]:off[3]].any() and np.isfinite(minv).all()
    inv, js = R.build_jacobi(R.precond_plan(n, rows, cols, "lower"), v, np.float64)
    np.testing.assert_array_equal(js, [bs[2] + 4, 1])
    assert inv[bs[2] + 4] == 0.0 and np.isfinite(inv).all()


# ---- the host plan -------------------------------------------------------------------------------------------
def _plan_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("dups", "full"):
        sizes = [1, 3, 9, 32, 3, 1, 9]
        n = sum(sizes)
        i, j = np.nonzero(np.tril(rng.random((n, n)) < 0.5))
        rows, cols, _ = duplicated(i.astype(np.int64), j.astype(np.int64), rng, max_dup=4, full=(name == "full"))
        return n, rows, cols, sizes, name if name == "full" else "lower"
    if name == "ones":
        n, rows, cols, _ = SP.grid_entries(4, 0.0)
        return n, rows, cols, None, "lower"
    if name == "nodiag":  # params without a single entry in their diagonal block
        return 6, np.array([5, 3]), np.array([0, 1]), [2, 2, 2], "lower"
    raise KeyError(name)


@pytest.mark.parametrize("name", ["dups", "full", "ones", "nodiag"])
def test_plan_tables_match_the_restatement(name):
    n, rows, cols, sizes, tri = _plan_case(name)
    pat = S.SymmetricPattern(rows, cols, n, param_sizes=sizes, triangle=tri)
    for kind, bsizes in (("jacobi", None), ("block_jacobi", pat.param_sizes)):
        want = R.precond_plan(n, rows, cols, tri, bsizes)
        got = pat.product.cgPrecondTable(kind)
        for g, w in zip(got[:4], want):
            assert g.dtype == np.int32
            np.testing.assert_array_equal(g, w)
        widths = np.diff(want[0])
        assert got[4] == {"blocks": len(widths), "items": len(want[2]), "inverse_elems": int((widths ** 2).sum()),
                          "max_width": int(widths.max())}
        # ascending entry index inside every block, every position inside the lower triangle of its block
        for b in range(len(widths)):
            e, p = got[2][got[1][b]:got[1][b + 1]], got[3][got[1][b]:got[1][b + 1]]
            assert (np.diff(e) > 0).all()
            assert ((p // widths[b]) >= (p % widths[b])).all() and (p < widths[b] ** 2).all()
    if name in ("dups", "full"):
        assert max(sizes) == 32 and got[4]["max_width"] == 32


def test_width_33_is_refused_by_name():
    sizes = [2, 33, 1]
    n = sum(sizes)
    d = np.arange(n)
    pat = S.SymmetricPattern(d, d, n, param_sizes=sizes)
    with pytest.raises(RuntimeError, match=r"param 1 has 33 scalars"):
        pat.product.cgPrecondTable("block_jacobi")
    assert pat.product.cgPrecondTable("jacobi")[4]["blocks"] == n
    with pytest.raises(ValueError, match="param 1 has 33"):
        R.precond_plan(n, d, d, "lower", sizes)
    with pytest.raises(ValueError, match="jacobi"):
        pat.product.cgPrecondTable("ilu")


# ---- refusals that need no device ----------------------------------------------------------------------
def test_settings_refusals():
    for kw in ({"tol": -1.0}, {"tol": float("nan")}, {"tol": "1"}, {"max_steps": -1}, {"max_steps": 1.5},
               {"max_steps": True}, {"check_every": 0}, {"check_every": 2.0}):
        args = {"tol": 1e-10, "max_steps": 10, "check_every": 8}
        args.update(kw)
        with pytest.raises(ValueError, match=list(kw)[0]):
            CG.check_settings("solve_cg", **args)
    CG.check_settings("solve_cg", 0, 0, None)
    with pytest.raises(TypeError, match="solver"):
        pcg.DevicePCG(lambda r: r, lambda p: p)
    with pytest.raises(ValueError, match="check_every"):
        pcg.DevicePCG(lambda r: r, lambda p: p, check_every=0, solver=object())


def test_work_bytes_and_state_words():
    import ctypes
    lib = _lib.load()
    sol = SP.pattern("blocks").solver
    words = ctypes.c_int64(0)
    assert lib.bsp_cg_state_words(ctypes.byref(words)) == 0 and words.value == 12
    for n, q in ((0, 1), (1, 1), (1024, 3), (1025, 3), (5000, 2)):
        need = ctypes.c_int64(0)
        assert lib.bsp_cg_work_bytes(sol._h, ctypes.c_int64(n), ctypes.c_int64(q), ctypes.byref(need)) == 0
        assert need.value == 16 * q * max(1, (n + 1023) // 1024) + (4 * max(n, 1) + 15) // 16 * 16
    need = ctypes.c_int64(0)
    assert lib.bsp_cg_work_bytes(sol._h, ctypes.c_int64(4), ctypes.c_int64(0), ctypes.byref(need)) != 0
    assert b"q = 0" in lib.bsp_last_error()
    assert lib.bsp_cg_work_bytes(None, ctypes.c_int64(4), ctypes.c_int64(1), ctypes.byref(need)) != 0
    # the pieces refuse their arguments before any device work
    z = ctypes.c_void_p(0)
    i64 = ctypes.c_int64
    assert lib.bsp_cg_alpha_f64(sol._h, i64(4), i64(1), z, z, z, z) != 0
    assert b"workspace pointer is NULL" in lib.bsp_last_error()
    assert lib.bsp_cg_alpha_f64(sol._h, i64(4), i64(1), z, z, ctypes.c_void_p(24), z) != 0
    assert b"not 16-byte aligned" in lib.bsp_last_error()
    assert lib.bsp_cg_alpha_f64(sol._h, i64(4), i64(1), z, z, ctypes.c_void_p(32), z) != 0
    assert b"state pointer is NULL" in lib.bsp_last_error()
    assert lib.bsp_cg_alpha_f64(sol._h, i64(4), i64(1), z, z, ctypes.c_void_p(32), ctypes.c_void_p(4096)) != 0
    assert b"the p pointer of batch member 0 is NULL" in lib.bsp_last_error()
    assert lib.bsp_cg_alpha_f64(sol._h, i64(-1), i64(1), z, z, ctypes.c_void_p(32), ctypes.c_void_p(4096)) != 0
    assert b"n = -1" in lib.bsp_last_error()
    p = ctypes.c_void_p(1 << 20)
    assert lib.bsp_cg_update_f64(sol._h, i64(4), i64(1), p, ctypes.c_void_p((1 << 20) + 64), ctypes.c_void_p((1 << 20) + 128),
                                 ctypes.c_void_p((1 << 20) + 136), ctypes.c_int32(1), ctypes.c_void_p(32),
                                 ctypes.c_void_p(4096)) != 0
    assert b"aliases" in lib.bsp_last_error()
    assert lib.bsp_cg_init_f64(sol._h, i64(4), i64(1), p, ctypes.c_void_p((1 << 20) + 64), ctypes.c_void_p((1 << 20) + 128),
                               ctypes.c_double(-1.0), i64(5), ctypes.c_int32(1), ctypes.c_void_p(32),
                               ctypes.c_void_p(4096)) != 0
    assert b"tol" in lib.bsp_last_error()
    other = SP.pattern("dups")
    assert lib.bsp_cg_precond_build_f64(sol._h, other.product._h, ctypes.c_int32(1), p, ctypes.c_void_p((1 << 20) + 4096),
                                        ctypes.c_void_p(32), ctypes.c_void_p(4096)) != 0
    assert b"another solver" in lib.bsp_last_error()
    assert lib.bsp_cg_precond_build_f64(sol._h, SP.pattern("blocks").product._h, ctypes.c_int32(7), p,
                                        ctypes.c_void_p((1 << 20) + 4096), ctypes.c_void_p(32), ctypes.c_void_p(4096)) != 0
    assert b"kind" in lib.bsp_last_error()
