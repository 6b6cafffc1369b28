"""CPU: the host map of the implicit Schur elimination against the numpy restatement
(schur_ref.py): every list of the map on the bundle-adjustment like case, the narrow and the wide eliminated params
and the hub case; every refusal with its message; and the restatement alone: reduce, conjugate gradient on S and
back-substitution in float64 against the dense solution of the damped normal equations."""
import ctypes
import re

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import sparse as S

import schur_ref as SR

NAMES = ("bsp_jac_schur_create", "bsp_jac_schur_destroy", "bsp_jac_schur_info", "bsp_jac_schur_table",
         "bsp_jac_schur_precond_info") + tuple(
    "bsp_jac_schur_%s_%s%s" % (op, b, sfx) for op in ("build", "mv", "reduce", "back", "precond_build", "precond_apply")
    for b in ("", "batched_") for sfx in ("f64", "f32"))


def test_symbols_are_declared_and_exported():
    import os
    lib = B._lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(B.__file__))), "include",
                               "baspacho_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", SR.TABLE_CASES + ["bidiag_255"])
def test_every_list_matches_the_restatement(name):
    c, elim, jop, sch = SR.operator(name)
    ref, got = SR.tables(c, elim), sch.table()
    kept_blocks, kept_params = ref.pop("_kept_blocks")
    want = kept_blocks()
    bs, bw, ist, par, ka, kb, pos = sch.map.keptBlockTable()
    for a, b in zip((bs, bw, ist, ka, kb, pos, par), want + (kept_params,)):
        assert a.dtype == np.int32 and np.array_equal(a, b), (name, "kept blocks")
    pinfo = sch.map.precondInfo("block_jacobi")
    assert (pinfo["blocks"], pinfo["items"]) == (len(kept_params), len(want[3]))
    assert pinfo["inverse_elems"] == int((want[1].astype(np.int64) ** 2).sum()) and pinfo["max_width"] == int(want[1].max())
    jinfo = sch.map.precondInfo("jacobi")
    assert (jinfo["blocks"], jinfo["items"], jinfo["inverse_elems"]) == (sch.nK, 0, sch.nK)
    assert set(ref) == set(got)
    for key, want in ref.items():
        parts = zip(got[key], want) if isinstance(want, tuple) else [(got[key], want)]
        for a, b in parts:
            assert a.dtype == np.int32 and np.array_equal(a, b), (name, key)
    info = sch.info()
    sizes = np.ones(c["n"], dtype=np.int64) if c["param_sizes"] is None else c["param_sizes"]
    w = sizes[sorted(elim)]
    assert (info["nnz"], info["m"], info["n"]) == (len(c["rows"]), c["m"], c["n"])
    assert (info["n_kept"], info["n_elim"], info["elim_params"]) == (c["n"] - int(w.sum()), int(w.sum()), len(elim))
    assert info["free_rows"] == len(ref["free_rows"]) and info["group_rows"] == len(ref["group_row"])
    assert info["free_rows"] + info["group_rows"] == c["m"]
    assert info["max_elim_width"] == int(w.max()) and info["max_group"] == int(np.diff(ref["group_start"]).max())
    assert info["kept_entries"] + info["elim_entries"] == len(c["rows"])
    for key in ("rows_kept", "rows_elim", "cols_elim", "cols_kept"):
        assert info["long_" + key] == len(ref[key][3]) == int((np.diff(ref[key][0]) > 64).sum())
    assert info["block_items"] == len(ref["item_a"]) and info["inverse_elems"] == int((w * w).sum())
    words = sum(len(x) for key in ("rows_kept", "rows_elim", "cols_elim", "cols_kept") for x in ref[key])
    words += sum(len(ref[key]) for key in ("elim_off", "kept_scalar", "elim_scalar", "group_start", "group_row", "free_rows"))
    assert info["map_bytes"] == 4 * words


def test_hub_case_has_the_runs_it_is_for():
    c, elim = SR.case("hub")
    t = SR.tables(c, elim)
    assert np.diff(t["group_start"]).tolist() == [1, 63, 64, 65, 129, 256, 257, 0]  # the last param has no rows
    kept_cols = np.diff(t["cols_kept"][0])
    assert kept_cols[0] == 65 and kept_cols[1] == 129 and t["cols_kept"][3].tolist() == [0, 1]
    elim_cols = np.diff(t["cols_elim"][0])
    assert 65 in elim_cols.tolist() and elim_cols[-1] == 0
    per_row_kept, per_row_elim = np.diff(t["rows_kept"][0]), np.diff(t["rows_elim"][0])
    assert ((per_row_kept == 0) & (per_row_elim > 0)).sum() == 1  # eliminated entries only
    assert ((per_row_kept > 0) & (per_row_elim == 0)).sum() == 65 + 129  # kept entries only
    assert ((per_row_kept == 0) & (per_row_elim == 0)).sum() == 1  # the empty row
    assert len(t["free_rows"]) == 65 + 129 + 1
    assert t["block_width"].tolist() == [1, 2, 3, 1, 2, 1, 8, 1]


def test_the_eliminated_params_are_taken_in_ascending_order():
    c, elim, jop, sch = SR.operator("w1")
    other = S.JacobianSchur(jop, np.asarray(elim[::-1], dtype=np.int64))
    a, b = sch.table(), other.table()
    for key in a:
        for x, y in (zip(a[key], b[key]) if isinstance(a[key], tuple) else [(a[key], b[key])]):
            assert np.array_equal(x, y), key


# ---- refusals -----------------------------------------------------------------------------------------------
def test_refusals_of_the_map():
    c, elim, jop, sch = SR.operator("ba")
    num = len(c["param_sizes"])
    with pytest.raises(RuntimeError, match=r"jacobian schur: no param is eliminated; use the plain least squares"):
        S.JacobianSchur(jop, np.zeros(0, dtype=np.int64))
    with pytest.raises(RuntimeError, match=r"jacobian schur: eliminate\[1\] = %d is out of range \[0, %d\)" % (num, num)):
        S.JacobianSchur(jop, [1, num])
    with pytest.raises(RuntimeError, match=r"jacobian schur: eliminate\[0\] = -1 is out of range"):
        S.JacobianSchur(jop, [-1])
    with pytest.raises(RuntimeError, match=r"jacobian schur: eliminate\[2\] = 1 is given twice"):
        S.JacobianSchur(jop, [1, 2, 1])
    with pytest.raises(RuntimeError, match=r"jacobian schur: eliminated param 0 has 9 scalars; an eliminated param has "
                                           r"at most 8"):
        S.JacobianSchur(jop, [1, 0])
    with pytest.raises(RuntimeError, match=r"jacobian schur: every param is eliminated; nothing is kept"):
        S.JacobianSchur(SR.operator("w1")[2], np.arange(10))
    # a Jacobian whose rows 0 and 2 touch two scalars each: eliminating both scalars of such a row is refused
    rows, cols = [0, 0, 1, 2, 2], [0, 2, 1, 1, 2]
    two = S.JacobianOperator(rows, cols, 3, 3)
    case = {"rows": np.array(rows), "cols": np.array(cols), "m": 3, "n": 3, "param_sizes": None}
    assert SR.row_conflict(case, [0, 2]) == (0, 0, 2) and SR.row_conflict(case, [1, 2]) == (2, 1, 2)
    with pytest.raises(RuntimeError, match=r"jacobian schur: row 0 has entries in the eliminated params 0 and 2; a row "
                                           r"may touch one eliminated param only"):
        S.JacobianSchur(two, [2, 0])
    with pytest.raises(RuntimeError, match=r"jacobian schur: row 2 has entries in the eliminated params 1 and 2"):
        S.JacobianSchur(two, [1, 2])
    assert S.JacobianSchur(two, [0]).nK == 2
    with pytest.raises(TypeError, match="jop must be a JacobianOperator"):
        S.JacobianSchur(two.product, [0])
    other = S.JacobianOperator(rows, cols, 3, 3)
    with pytest.raises(ValueError, match="product must be a JacobianProduct of this solver"):
        two.solver.jacobianSchur(other.product, [0])


def test_refusals_of_the_c_entries():
    lib = B._lib.load()
    c, elim, jop, sch = SR.operator("w1")
    h = ctypes.c_void_p()
    assert lib.bsp_jac_schur_create(None, ctypes.c_int64(0), None, ctypes.byref(h)) != 0
    assert "NULL product or output" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_create(jop.product._h, ctypes.c_int64(2), None, ctypes.byref(h)) != 0
    assert "the list of eliminated params is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_info(None, None) != 0
    assert lib.bsp_jac_schur_table(None, ctypes.c_int32(0), None, None, None, None) != 0
    assert lib.bsp_jac_schur_table(sch.map._h, ctypes.c_int32(10), None, None, None, None) != 0
    assert "unknown part 10" in lib.bsp_last_error().decode()
    out = (ctypes.c_int64 * 5)()
    assert lib.bsp_jac_schur_precond_info(sch.map._h, ctypes.c_int32(3), out) != 0
    assert "unknown kind 3" in lib.bsp_last_error().decode()
    wide = S.JacobianOperator([0, 1], [0, 40], 2, 42, param_sizes=[8, 33, 1])
    with pytest.raises(RuntimeError, match=r"jacobian schur: kept param 1 has 33 scalars; block_jacobi takes params of at "
                                           r"most 32"):
        S.JacobianSchur(wide, [0]).map.precondInfo("block_jacobi")
    assert S.JacobianSchur(wide, [0]).map.precondInfo("jacobi")["blocks"] == 34
    with pytest.raises(ValueError, match="kind must be 'jacobi' or 'block_jacobi'"):
        sch.map.precondInfo("fsai")
    assert lib.bsp_jac_schur_table(sch.map._h, ctypes.c_int32(4), None, None, None, None) != 0
    assert "an output array is NULL" in lib.bsp_last_error().decode()
    # the device entries check their operands before any device work
    assert lib.bsp_jac_schur_mv_f64(jop.solver._h, None, ctypes.c_int64(1), None, None, None, None, None, None, None) != 0
    assert "the map is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_mv_f64(jop.solver._h, sch.map._h, ctypes.c_int64(1), None, None, None, None, None, None,
                                    None) != 0
    assert "schurMv: the values pointers are NULL" in lib.bsp_last_error().decode() or \
        "schurMv: the values pointer of batch member 0 is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_build_f32(jop.solver._h, sch.map._h, None, None, None, None, None) != 0
    assert "schurBuild: the workspace pointer is NULL" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_schur_reduce_f64(jop.solver._h, sch.map._h, ctypes.c_int64(0), None, None, None, None, None) != 0
    assert "schurReduce" in lib.bsp_last_error().decode()
    other = S.JacobianOperator([0], [0], 1, 1)
    assert lib.bsp_jac_schur_back_f64(other.solver._h, sch.map._h, ctypes.c_int64(1), None, None, None, None, None,
                                      None) != 0
    assert "schurBack: the map was built on another solver" in lib.bsp_last_error().decode()


# ---- the restatement alone ----------------------------------------------------------------------------------
TOL = 1e-12


@pytest.mark.parametrize("name", SR.DENSE_CASES)
@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
@pytest.mark.parametrize("which", ["r", "c", "rc"])
def test_the_model_reaches_the_dense_solution(name, which, precond):
    """the bound is kappa(N) tol on the relative error of the full x, kappa(N) <= 100 from the dense matrix"""
    import cgls_ref as C
    c, elim = SR.case(name)
    rng = np.random.default_rng(7)
    r = rng.uniform(-1, 1, (c["m"], 2)) if "r" in which else None
    cv = rng.uniform(-1, 1, (c["n"], 2)) if "c" in which else None
    mdl = SR.model(name, np.float64, True)
    xd, Nm = C.dense_solution(c, r=r, cvec=cv, damping_ab=SR.DENSE_DAMPING)
    kappa = np.linalg.cond(Nm)
    assert kappa <= 100, kappa
    x, st = mdl.solve(r=r, c=cv, precond=precond, tol=TOL, max_steps=200)
    assert (st["stop"] == 1).all() and mdl.status.tolist() == [-1, 0]
    assert precond is None or mdl.precond_status.tolist() == [-1, 0]
    err = np.linalg.norm(x - xd, axis=0) / np.linalg.norm(xd, axis=0)
    print("%s %s %s: kappa %.1f, iterations %s, error %s, bound %.1e" % (name, which, precond, kappa, st["iterations"], err,
                                                                        kappa * TOL))
    assert (err <= kappa * TOL).all(), (err, kappa * TOL)


@pytest.mark.parametrize("name", SR.DENSE_CASES)
def test_the_model_product_is_the_dense_reduced_matrix(name):
    mdl = SR.model(name, np.float64, True)
    Sd, _ = mdl.dense_s()
    p = np.random.default_rng(8).uniform(-1, 1, (mdl.nK, 3))
    assert np.allclose(mdl.mv(p), Sd @ p, rtol=1e-12, atol=1e-12)
    # reduce and back-substitution solve the full system when x_k is exact
    g = np.random.default_rng(9).uniform(-1, 1, (mdl.n, 2))
    _, Nm = mdl.dense_s()
    xk = np.linalg.solve(Sd, mdl.reduce(g))
    assert np.allclose(mdl.back(g, xk), np.linalg.solve(Nm, g), rtol=1e-11, atol=1e-12)


def test_a_param_without_rows_is_a_bad_block_without_damping():
    c, elim = SR.case("hub")
    mdl = SR.model("hub", np.float64, False)
    assert mdl.status.tolist() == [int(mdl.t["elim_scalar"][-1]), 1]
    assert (mdl.binv[mdl.block_off[-2]:] == 0).all()
    assert SR.model("hub", np.float64, True).status.tolist() == [-1, 0]
