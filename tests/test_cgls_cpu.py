"""CPU: the host map of the matrix-free least squares against the numpy restatement
(cgls_ref.py): the run lists of the rows and columns with their long runs, the plan of the diagonal blocks of
J^T J, every refusal; and the restatement alone: cgls_model in float64 against the dense solution of the damped
normal equations within the bound the GPU suite uses, and the concatenated fold of the curvature."""
import ctypes

import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import sparse as S

import cgls_ref as C
import normal_eq_ref as N

CASES = N.CASES + ["hub"]


def _sizes(c):
    return np.ones(c["n"], dtype=np.int64) if c["param_sizes"] is None else np.asarray(c["param_sizes"])


@pytest.mark.parametrize("name", CASES)
def test_run_lists_match_the_restatement(name):
    c, op = C.operator(name)
    info = op.product.info()
    for which, keys, other, num in (("rows", c["rows"], c["cols"], c["m"]), ("cols", c["cols"], c["rows"], c["n"])):
        ref = C.run_list(keys, other, num)
        got = op.product.runTable(which)
        for a, b in zip(got, ref):
            assert a.dtype == np.int32 and np.array_equal(a, b), (name, which)
        lens = np.diff(ref[0])
        assert info["max_" + which[:3]] == (int(lens.max()) if len(lens) else 0)
        assert info["long_" + which] == len(ref[3]) == int((lens > 64).sum())
        assert info[which[:3] + "_bytes"] == 4 * (num + 1 + 2 * len(keys) + len(ref[3]))
    assert (info["nnz"], info["m"], info["n"]) == (len(c["rows"]), c["m"], c["n"])


@pytest.mark.parametrize("name", CASES)
def test_block_plan_matches_the_restatement(name):
    c, op = C.operator(name)
    sizes = _sizes(c)
    if sizes.max(initial=0) > 32:
        with pytest.raises(RuntimeError, match=r"param 0 has 72 scalars; block_jacobi takes blocks of at most 32"):
            op.product.blockTable()
        return
    ref = C.block_plan(c["rows"], c["cols"], c["m"], sizes)
    got = op.product.blockTable()
    for a, b in zip(got, ref):
        assert a.dtype == np.int32 and np.array_equal(a, b), name
    info = op.product.precondInfo("block_jacobi")
    assert info["blocks"] == len(sizes) and info["items"] == len(ref[2])
    assert info["inverse_elems"] == int((sizes * sizes).sum()) and info["max_width"] == int(sizes.max(initial=0))
    assert info["device_bytes"] == 4 * (2 * (len(sizes) + 1) + c["n"] + 3 * len(ref[2])) + 8 * (len(sizes) + 1)
    jac = op.product.precondInfo("jacobi")
    assert (jac["blocks"], jac["items"], jac["inverse_elems"]) == (c["n"], 0, c["n"])


def test_hub_case_has_the_runs_it_is_for():
    c = C.hub()
    per_col, per_row = np.bincount(c["cols"], minlength=c["n"]), np.bincount(c["rows"], minlength=c["m"])
    assert sorted(per_col[per_col >= 64].tolist()) == [64, 65, 128, 129] and per_col[-1] == 0
    assert per_row.max() == 65 and (c["m"], c["n"]) == (130, 94)
    assert c["param_sizes"].tolist() == [1, 3, 9, 32, 2] * 2
    info = C.operator("hub")[1].product.info()
    assert info["long_cols"] == 3 and info["long_rows"] == 1  # 64 entries are not a long run


def test_the_pattern_builds_the_same_map_on_its_own_solver():
    c, pat = N.pattern("blocks_elim")
    op = pat.operator
    assert op is pat.operator and op.solver is pat.solver and op.product.solver is pat.solver
    for which in ("rows", "cols"):
        for a, b in zip(op.product.runTable(which), C.operator("blocks_elim")[1].product.runTable(which)):
            assert np.array_equal(a, b)
    # the blocks are the params in the caller's order, whatever the solver's elimination order is
    for a, b in zip(op.product.blockTable(), C.block_plan(c["rows"], c["cols"], c["m"], c["param_sizes"])):
        assert np.array_equal(a, b)


def test_creating_the_map_builds_nothing_of_the_pair_count():
    # 40 dense rows over 3000 columns: P = 40 * 3000 * 3001 / 2 = 1.8e8 pairs, 1.4 GB of forward map alone; the
    # product map has 2 * (nnz + runs) words.  Block-Jacobi over scalar params takes the nnz self-pairs only
    m, n = 40, 3000
    rows, cols = np.repeat(np.arange(m), n), np.tile(np.arange(n), m)
    op = S.JacobianOperator(rows, cols, m, n)
    info = op.product.info()
    assert info["row_bytes"] + info["col_bytes"] == 4 * (m + 1 + n + 1 + 4 * m * n + m)
    assert op.product.precondInfo("block_jacobi")["items"] == m * n


# ---- refusals -----------------------------------------------------------------------------------------------
def test_refusals_of_the_map():
    with pytest.raises(RuntimeError, match=r"jacobian product: entry 1 at \(2, 0\) is out of range \[0, 2\) x \[0, 3\)"):
        S.JacobianOperator([0, 2], [0, 0], 2, 3)
    with pytest.raises(RuntimeError, match=r"jacobian product: entry 0 at \(0, 3\) is out of range"):
        S.JacobianOperator([0, 1], [3, 0], 2, 3)
    with pytest.raises(RuntimeError, match=r"jacobian product: entry 1 at \(-1, 0\) is out of range"):
        S.JacobianOperator([0, -1], [0, 0], 2, 3)
    with pytest.raises(RuntimeError, match=r"jacobian product: entry 3 at \(1, 2\) repeats the position of entry 1; "
                                           r"duplicate Jacobian entries are not summed"):
        S.JacobianOperator([0, 1, 0, 1, 1], [0, 2, 1, 2, 2], 2, 3)
    with pytest.raises(RuntimeError, match=r"jacobian product: m = -1 is outside \[0, 2\^31\)"):
        S.JacobianOperator([], [], -1, 3)
    with pytest.raises(ValueError, match="JacobianOperator: 2 rows for 1 cols"):
        S.JacobianOperator([0, 1], [0], 2, 3)
    with pytest.raises(ValueError, match="param sizes must be >= 1 and sum to n = 3"):
        S.JacobianOperator([0], [0], 2, 3, param_sizes=[2, 2])


def test_refusals_of_the_plan_and_the_tables():
    lib = B._lib.load()
    wide = S.JacobianOperator([0, 1], [0, 40], 2, 41, param_sizes=[8, 33])
    with pytest.raises(RuntimeError, match=r"jacobian product: param 1 has 33 scalars; block_jacobi takes blocks of at "
                                           r"most 32"):
        wide.product.precondInfo("block_jacobi")
    assert wide.product.precondInfo("jacobi")["blocks"] == 41  # Jacobi does not ask for the blocks
    # the item count is checked, and stated, before anything of its size is allocated
    assert lib.bsp_jac_product_check_items(ctypes.c_int64(2 ** 31 - 1)) == 0
    assert lib.bsp_jac_product_check_items(ctypes.c_int64(2 ** 31)) != 0
    assert "take 2147483648 pairs of entries, outside [0, 2^31)" in lib.bsp_last_error().decode()
    op = C.operator("scalar")[1]
    with pytest.raises(ValueError, match="kind must be 'jacobi' or 'block_jacobi'"):
        op.product.precondInfo("fsai")
    with pytest.raises(ValueError, match="which must be 'rows' or 'cols'"):
        op.product.runTable("pairs")
    out = (ctypes.c_int64 * 5)()
    assert lib.bsp_cgls_precond_info(op.product._h, ctypes.c_int32(3), out) != 0
    assert "unknown kind 3" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_product_table(op.product._h, ctypes.c_int32(5), None, None, None, None, None) != 0
    assert "unknown part 5" in lib.bsp_last_error().decode()
    assert lib.bsp_jac_product_table(None, ctypes.c_int32(0), None, None, None, None, None) != 0
    assert lib.bsp_jac_product_info(None, None) != 0
    assert lib.bsp_jac_product_create(None, ctypes.c_int64(1), ctypes.c_int64(0), None, None, None) != 0
    need = ctypes.c_int64(0)
    assert lib.bsp_cgls_work_bytes(op.solver._h, op.product._h, ctypes.c_int64(0), ctypes.byref(need)) != 0
    assert "q = 0" in lib.bsp_last_error().decode()
    assert lib.bsp_cgls_work_bytes(op.solver._h, op.product._h, ctypes.c_int64(3), ctypes.byref(need)) == 0
    mp, np_ = (op.m + 1023) // 1024, (op.n + 1023) // 1024
    assert need.value == 3 * max(mp + np_, 2 * np_, 1) * 16 + (4 * op.n + 15) // 16 * 16


# ---- the restatement alone --------------------------------------------------------------------------------------
DENSE_CASES, DENSE_DAMPING, dense_case = C.DENSE_CASES, C.DENSE_DAMPING, C.dense_case
F64_BOUND = 1e-10  # kappa * tol = 100 * 1e-12


@pytest.mark.parametrize("name,scale", DENSE_CASES)
@pytest.mark.parametrize("precond", [None, "jacobi", "block_jacobi"])
def test_the_model_reaches_the_dense_solution(name, scale, precond):
    c, v = dense_case(name, scale)
    r = np.random.default_rng(5).uniform(-1, 1, (c["m"], 2))
    ab = DENSE_DAMPING
    xd, Nm = C.dense_solution(c, r=r, damping_ab=ab, values=v)
    kappa = np.linalg.cond(Nm)
    assert kappa <= 100, kappa
    x, st, status = C.cgls_model(c, np.float64, r=r, damping_ab=ab, precond=precond, tol=1e-12, max_steps=200, values=v)
    assert (st["stop"] == 1).all() and (status is None or status.tolist() == [-1, 0])
    err = np.linalg.norm(x - xd, axis=0) / np.linalg.norm(xd, axis=0)
    print("%s %s: kappa %.1f, iterations %s, error %s" % (name, precond, kappa, st["iterations"], err))
    assert (err < F64_BOUND).all(), err


def test_the_curvature_fold_is_one_list_not_two():
    rng = np.random.default_rng(6)
    t, p, d = rng.uniform(-1, 1, (5000, 2)), rng.uniform(-1, 1, (4100, 2)), rng.uniform(0.1, 1, 4100)
    one = C.delta(t, p, d)
    two = C.fold_parts(C.partials(t * t)) + C.fold_parts(C.partials((p * p) * d[:, None]))
    assert (one != two).all() and np.allclose(one, two, rtol=1e-14)
    # without damping the list is t.t's alone: cg_ref's dot
    import cg_ref as R
    assert np.array_equal(C.delta(t, p, None), R.dot(t, t))
    # ten partials: thread u of the second pass holds partial u, folded pairwise from the top
    parts = np.concatenate([C.partials(t * t), C.partials((p * p) * d[:, None])])
    assert parts.shape == (10, 2)
    s = [parts[u] for u in range(10)]
    assert np.array_equal(one, (((s[0] + s[8]) + s[4]) + (s[2] + s[6])) + (((s[1] + s[9]) + s[5]) + (s[3] + s[7])))


def test_the_epilogues_omit_absent_operands():
    dt = np.float32
    total = np.array([[-0.0], [1.5]], dtype=dt)
    assert np.array_equal(np.signbit(C.epilogue_normal(total, None, None, None)), [[True], [False]])
    zero = np.zeros((2, 1), dtype=dt)
    assert not np.signbit(C.epilogue_normal(total, None, None, zero))[0, 0]  # -0 + 0 = +0: a zero is not "absent"
    assert np.signbit(C.epilogue_residual(None, np.array([[0.0]], dtype=dt)))[0, 0]
    assert not np.signbit(C.epilogue_residual(np.array([[0.0]], dtype=dt), np.array([[0.0]], dtype=dt)))[0, 0]
