"""CPU: the map of the products with a symmetric matrix given as entries and the host
models the GPU tests compare against, without a GPU.  rowTable() and info() must equal the term lists stated
one entry at a time (sym_product_ref.row_terms) on every case, refusals must name the entry, the models of
mv and outer must stay inside the bounds of a sequential sum against np.longdouble, and the host model of
solve_refined must reach float64 accuracy on the grid cases (its error is the GPU's yardstick)."""
import os
import re

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import _lib
from baspacho_amd import sparse as S
import sym_product_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bsp_sym_product_create", "bsp_sym_product_destroy", "bsp_sym_product_info", "bsp_sym_product_row_table"] + \
    ["bsp_sym_product_%s%s_%s" % (op, b, t) for op in ("mv", "outer") for b in ("", "_batched") for t in ("f64", "f32")]


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % name, header), name
        assert hasattr(lib, name), name


def test_names_are_exported():
    for name in ("matvec", "quad_form", "log_prob", "solve_refined"):
        assert name in S.__all__ and callable(getattr(S, name)) and name in S.__doc__
    assert "SymProduct" in B.__all__ and isinstance(B.SymProduct, type)
    assert callable(B.Solver.symProduct)


@pytest.mark.parametrize("name", R.CASES)
def test_row_table_matches_reference(name):
    c, pat = R.case(name), R.pattern(name)
    prod = pat.product
    assert isinstance(prod, B.SymProduct) and prod is pat.product and prod.solver is pat.solver
    start, entry, index, info = R.row_terms(c["n"], c["rows"], c["cols"], c["triangle"])
    got = prod.rowTable()
    for g, w in zip(got, (start, entry, index)):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, w)
    gi = prod.info()
    for key, val in info.items():
        assert gi[key] == val, (key, gi)
    n_long = info["long_rows"]
    assert gi["device_bytes"] == 4 * (c["n"] + 1 + 2 * info["terms"] + n_long + 2 * len(c["rows"]))
    # the same through the solver, which does not care whether it stores the elements
    other = pat.solver.symProduct(c["rows"], c["cols"], c["triangle"])
    np.testing.assert_array_equal(other.rowTable()[1], entry)


def test_cases_cover_what_they_claim():
    lens = {name: np.diff(R.row_terms(R.case(name)["n"], R.case(name)["rows"], R.case(name)["cols"],
                                      R.case(name)["triangle"])[0]) for name in R.CASES}
    assert list(lens["one"]) == [1] and lens["empty"].sum() == 0 and len(lens["empty"]) == 5
    assert list(np.nonzero(lens["gaps"] == 0)[0]) == [0, 1, 3, 4, 6, 8]
    for t in R.ARROWS:
        assert lens["arrow%d" % t][-1] == t and lens["arrow%d" % t][:-1].max() == 2
    full = R.case("full")
    assert np.any(full["rows"] < full["cols"])
    for name in ("dups", "full"):
        c = R.case(name)
        _, count = np.unique(c["rows"] * c["n"] + c["cols"], return_counts=True)
        assert 2 <= count.max() <= 8
    assert sorted(set(R.case("blocks")["param_sizes"])) == [1, 2, 3, 4]
    assert R.pattern("arrow65").product.info()["long_rows"] == 1 and R.pattern("arrow64").product.info()["long_rows"] == 0


def test_lazy_product():
    c = R.case("gaps")
    pat = S.SymmetricPattern(c["rows"], c["cols"], c["n"])
    assert pat._product is None
    assert pat.product.nnz == len(c["rows"]) and pat._product is not None


def test_refusals_name_the_entry():
    sol = R.pattern("dups").solver
    n = sol.order()
    with pytest.raises(RuntimeError, match=r"entry 2 at \(%d, 0\) is out of range" % n):
        sol.symProduct([0, 1, n], [0, 0, 0])
    with pytest.raises(RuntimeError, match=r"entry 1 at \(0, -1\) is out of range"):
        sol.symProduct([0, 0], [0, -1])
    with pytest.raises(RuntimeError, match=r"entry 1 at \(3, %d\) is out of range" % (n + 4)):
        sol.symProduct([0, 3], [0, n + 4], "full")
    with pytest.raises(RuntimeError, match=r"entry 1 at \(2, 5\) has row < col"):
        sol.symProduct([1, 2, 3], [0, 5, 9], "lower")
    # the same entry in full mode is skipped, not refused; the later one is named
    prod = sol.symProduct([1, 2], [0, 5], "full")
    assert prod.info()["kept"] == 1 and prod.info()["terms"] == 2
    with pytest.raises(ValueError, match="triangle"):
        sol.symProduct([0], [0], "upper")
    with pytest.raises(ValueError, match="rows for"):
        sol.symProduct([0, 1], [0])


def test_product_keeps_its_solver():
    c = R.case("gaps")
    pat = S.SymmetricPattern(c["rows"], c["cols"], c["n"])
    prod = pat.solver.symProduct(c["rows"], c["cols"])
    del pat
    assert prod.solver.order() == c["n"] and prod.info()["nnz"] == len(c["rows"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", R.CASES)
def test_mv_model_within_sequential_sum_bound(name, dtype):
    c = R.case(name)
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(3)
    v = c["values"].astype(dtype)
    for q in (None, 3):
        x = rng.uniform(-1, 1, (n,) if q is None else (n, q)).astype(dtype)
        got = R.mv_model(n, rows, cols, tri, v, x, dtype)
        assert got.dtype == dtype and got.shape == x.shape
        A = R.dense_ld(n, rows, cols, v)
        np.testing.assert_allclose(A.astype(np.float64), R.dense_user(n, rows, cols, v.astype(np.float64)),
                                   rtol=0, atol=1e-14)
        want = A @ x.astype(np.longdouble)
        bound = R.mv_bound(n, rows, cols, tri, v, x, dtype)
        assert np.all(np.abs(got.astype(np.longdouble) - want) <= bound), (name, q)
        empty = np.diff(R.row_terms(n, rows, cols, tri)[0]) == 0
        assert not np.any(got.reshape(n, -1)[empty]) and not np.any(np.signbit(got.reshape(n, -1)[empty]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", R.CASES)
def test_outer_model_within_bound(name, dtype):
    c = R.case(name)
    n, rows, cols, tri = c["n"], c["rows"], c["cols"], c["triangle"]
    rng = np.random.default_rng(4)
    for q in (None, 5):
        g = rng.uniform(-1, 1, (n,) if q is None else (n, q)).astype(dtype)
        x = rng.uniform(-1, 1, g.shape).astype(dtype)
        got = R.outer_model(n, rows, cols, tri, g, x, dtype)
        assert got.dtype == dtype and got.shape == (len(rows),)
        gl, xl = g.astype(np.longdouble).reshape(n, -1), x.astype(np.longdouble).reshape(n, -1)
        keep = rows >= cols
        r, cc = np.where(keep, rows, 0), np.where(keep, cols, 0)
        want = (gl[r] * xl[cc]).sum(1) + np.where(r != cc, (gl[cc] * xl[r]).sum(1), 0)
        want = np.where(keep, want, 0)
        assert np.all(np.abs(got.astype(np.longdouble) - want) <= R.outer_bound(n, rows, cols, g, x, dtype)), (name, q)
        assert not np.any(got[~keep])
        # every duplicate holds the full value
        key = rows[keep] * n + cols[keep]
        for k in np.unique(key):
            assert len(set(got[keep][key == k].tolist())) == 1


@pytest.mark.parametrize("name", list(R.GRIDS))
def test_refine_model_reaches_float64(name):
    """the yardstick of the GPU's solve_refined: the host loop against the longdouble-refined reference"""
    c = R.refine_case(name)
    print("%s: n %d cond %.1f  model %.3g  float64 direct %.3g  fp32 %.3g  GPU bound %.3g" % (
        name, c["n"], c["cond"], c["model_err"], c["direct_err"], c["fp32_err"], R.refine_bound(name)))
    assert abs(c["cond"] - R.GRID_COND[name]) < 1.0
    assert c["model_err"] <= 2e-15                      # float64 accuracy: eps times a small factor
    assert c["model_err"] <= 4 * c["direct_err"]        # as good as the float64 direct solve
    assert c["fp32_err"] >= 1e5 * c["model_err"]        # and far from the plain fp32 solve it starts from
    assert R.REFINE_MARGIN * c["model_err"] < R.REFINE_CAP
    # one correction fewer is still short of two: the loop does converge, it does not start converged
    assert R.rel_err(R.refine_model(c["A"], c["b"], 0), c["ref"]) == c["fp32_err"]
