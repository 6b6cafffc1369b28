"""CPU: the host plan of the "fsai" preconditioner (kind 3) against its numpy restatement
(fsai_ref.py), the restated build against an independent dense evaluation, what the preconditioner buys on the
ill-conditioned grid in the restated iteration, and the refusals that need no device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from baspacho_amd import _lib
from baspacho_amd import cg as CG
from baspacho_amd import sparse as S
from assembly_ref import dense_user
import cg_ref as R
import fsai_ref as F
import sym_product_ref as SP
from test_cg_cpu import _plan_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bsp_fsai_table", "bsp_fsai_check_sizes"] + \
    ["bsp_fsai_apply%s_%s" % (b, t) for b in ("", "_batched") for t in ("f64", "f32")]
TABLES = ("row_start", "cols", "item_start", "entry", "pos", "col_start", "col_pos", "col_row", "long_cols")


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "baspacho_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name), name
    assert CG.PRECOND_KINDS["fsai"] == 3 and "fsai" in S.solve_cg.__doc__


# ---- the host plan ------------------------------------------------------------------------------------------
def _case(name):
    """(n, rows, cols, triangle)"""
    if name in ("dups", "full", "ones", "nodiag"):
        n, rows, cols, _, tri = _plan_case(name)
        return n, np.asarray(rows), np.asarray(cols), tri
    if name == "banded33":
        rows, cols, _ = F.banded(80)
        return 80, rows, cols, "lower"
    if name.startswith("hub"):
        n, rows, cols, _ = F.hub(int(name[3:]))
        return n, rows, cols, "lower"
    if name == "one":
        return 1, np.array([0, 0]), np.array([0, 0]), "lower"
    raise KeyError(name)


@pytest.mark.parametrize("name", ["dups", "full", "ones", "nodiag", "banded33", "hub63", "hub64", "hub65", "one"])
def test_plan_tables_match_the_restatement(name):
    n, rows, cols, tri = _case(name)
    pat = S.SymmetricPattern(rows, cols, n, triangle=tri)
    got, want = pat.product.cgFsaiTable(), F.plan(n, rows, cols, tri)
    for key in TABLES:
        assert got[key].dtype == np.int32, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    widths = np.diff(want["row_start"])
    assert got["info"] == {"rows": n, "items": len(want["entry"]), "elems": int(widths.sum()),
                           "max_width": int(widths.max())}
    info = (ctypes.c_int64 * 4)()
    assert pat.product._lib.bsp_cg_precond_info(pat.product._h, ctypes.c_int32(3), info) == 0
    assert list(info) == [n, len(want["entry"]), int(widths.sum()), int(widths.max())]
    rs, its = got["row_start"], got["item_start"]
    for i in range(n):
        s = got["cols"][rs[i]:rs[i + 1]]
        assert s[-1] == i and (np.diff(s) > 0).all() and 1 <= len(s) <= 32
        e, p = got["entry"][its[i]:its[i + 1]], got["pos"][its[i]:its[i + 1]]
        assert (np.diff(e) > 0).all() and ((p // len(s)) >= (p % len(s))).all() and (p < len(s) ** 2).all()
    for j in range(n):  # every column list ascends in the row, holds j itself first and points at column j
        t = slice(got["col_start"][j], got["col_start"][j + 1])
        assert got["col_row"][t][0] == j and (np.diff(got["col_row"][t]) > 0).all()
        assert (got["cols"][got["col_pos"][t]] == j).all()
    if name == "banded33":  # every width 1 .. 32, then truncated rows that keep the 31 nearest scalars
        assert widths[:32].tolist() == list(range(1, 33)) and (widths[32:] == 32).all()
        for i in (32, 33, 34, 79):
            assert got["cols"][rs[i]:rs[i + 1]].tolist() == list(range(i - 31, i + 1))
    if name.startswith("hub"):  # 64 terms: still by a lane; 65 and 66: by a wave
        later = int(name[3:])
        assert got["col_start"][1] - got["col_start"][0] == later + 1
        assert got["long_cols"].tolist() == ([0] if later + 1 > 64 else [])
    if name in ("dups", "full"):
        assert widths.max() == 32  # rows truncated by the cap: not an error


def test_item_count_limit_is_checked_and_stated():
    lib = _lib.load()
    i64 = ctypes.c_int64
    assert lib.bsp_fsai_check_sizes(i64(5), i64((1 << 31) - 1)) == 0
    assert lib.bsp_fsai_check_sizes(i64(5), i64((1 << 31) + 7)) != 0
    msg = lib.bsp_last_error().decode()
    assert str((1 << 31) + 7) in msg and "items" in msg and "2^31" in msg
    assert lib.bsp_fsai_check_sizes(i64(1 << 31), i64(0)) != 0
    assert str(1 << 31) in lib.bsp_last_error().decode() and "elements of G" in lib.bsp_last_error().decode()
    with pytest.raises(ValueError, match=str((1 << 31) + 7)):
        F.check_sizes(5, (1 << 31) + 7)


# ---- the restated build ------------------------------------------------------------------------------------
# The largest relative deviation, per row of G (max |g - g_ref| / max |g_ref| over the row), of the restatement
# from the dense evaluation in np.longdouble, measured on these matrices: grid12 4.2e-15 (kappa_2 4e4: its local
# systems are the worst conditioned), bs_case 4.8e-15, banded33 5.3e-16, hub65 2.0e-16.  The only difference is
# the order of rounding, so the bound is 4 x the largest.
MEASURED_DEVIATION = 4.8e-15
DEVIATION_BOUND = 4 * MEASURED_DEVIATION


@pytest.mark.parametrize("name", ["grid12", "banded33", "bs_case", "hub65"])
def test_restated_rows_against_a_dense_evaluation(name):
    if name == "grid12":
        n, rows, cols, values, _ = F.grid12()
    elif name == "banded33":
        n = 80
        rows, cols, values = F.banded(n)
    elif name == "bs_case":
        rows, cols, values, _, n = R.bs_case()
    else:
        n, rows, cols, values = F.hub(65)
    pl = F.plan(n, rows, cols)
    G, status = F.build(pl, values, np.float64)
    np.testing.assert_array_equal(status, [-1, 0])
    want = F.dense_rows(pl, SP.dense_ld(n, rows, cols, values))
    rs = pl["row_start"]
    dev = max(float(np.abs(G[rs[i]:rs[i + 1]] - want[rs[i]:rs[i + 1]]).max() / np.abs(want[rs[i]:rs[i + 1]]).max())
              for i in range(n))
    print("fsai restatement against the dense evaluation,", name, ": largest relative deviation", dev,
          "bound", DEVIATION_BOUND)
    assert dev <= DEVIATION_BOUND
    # diag(G A G^T) = 1 in exact arithmetic
    A = dense_user(n, rows, cols, values)
    Gd = np.zeros((n, n))
    for i in range(n):
        Gd[i, pl["cols"][rs[i]:rs[i + 1]]] = G[rs[i]:rs[i + 1]]
    np.testing.assert_allclose(np.diag(Gd @ A @ Gd.T), 1.0, rtol=0, atol=1e-9)
    # float32 storage: the float64 row rounded once
    G32, _ = F.build(pl, values.astype(np.float32).astype(np.float64), np.float32)
    assert G32.dtype == np.float32


def test_bad_row_is_zeros_and_reported():
    rows, cols, values, _, n = R.bs_case()
    v = values.copy()
    scalar = 7
    v[int(np.nonzero((rows == scalar) & (cols == scalar))[0][0])] = -5.0
    pl = F.plan(n, rows, cols)
    G, status = F.build(pl, v, np.float64)
    rs = pl["row_start"]
    bad = [i for i in range(n) if not G[rs[i]:rs[i + 1]].any()]
    assert np.isfinite(G).all() and bad and status[1] == len(bad) and status[0] == scalar
    assert all(scalar in pl["cols"][rs[i]:rs[i + 1]] for i in bad)


# ---- what it buys --------------------------------------------------------------------------------------------
# iterations of the restated PCG to tol 1e-10 in float64 on the 12 x 12 grid of 3-wide params, shift 1e-3, as
# measured here: block_jacobi 152, fsai 73 (printed by the test; the assertion is the strict inequality)


def test_fewer_iterations_than_block_jacobi_on_the_ill_conditioned_grid():
    n, rows, cols, values, sizes = F.grid12()
    b = np.random.default_rng(1).uniform(-1, 1, n)
    _, st_b, _ = R.entries_model(n, rows, cols, values, b, np.float64, "block_jacobi", param_sizes=sizes, tol=1e-10,
                                 max_steps=1000)
    x, st_f, status = F.entries_model(n, rows, cols, values, b, np.float64, tol=1e-10, max_steps=1000)
    got = {"block_jacobi": int(st_b["iterations"][0]), "fsai": int(st_f["iterations"][0])}
    print("grid12 iterations", got)
    assert st_b["stop"][0] == R.CONVERGED and st_f["stop"][0] == R.CONVERGED and status.tolist() == [-1, 0]
    assert got["fsai"] < got["block_jacobi"]
    A = dense_user(n, rows, cols, values)
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) <= 1e-8


# ---- refusals that need no device ------------------------------------------------------------------------
def test_refusals_before_any_device_work():
    lib = _lib.load()
    pat = SP.pattern("blocks")
    sol, prod = pat.solver, pat.product
    n = pat.n
    i64, P, z = ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p(0)
    err = lambda: lib.bsp_last_error().decode()
    base = 1 << 20
    g, r, t, zz = (P(base + k * (1 << 16)) for k in range(4))
    work, state = P(32), P(4096)
    # kind 3 through the older entry: refused, and the message names the new one
    assert lib.bsp_cg_precond_f64(sol._h, prod._h, ctypes.c_int32(3), i64(n), i64(1), g, r, zz, work, state) != 0
    assert "bsp_fsai_apply" in err() and "fsai" in err()
    f = lib.bsp_fsai_apply_f64
    assert f(None, prod._h, i64(n), i64(1), g, r, t, zz, work, state) != 0 and "solver is NULL" in err()
    assert f(sol._h, None, i64(n), i64(1), g, r, t, zz, work, state) != 0 and "map is NULL" in err()
    assert f(sol._h, SP.pattern("dups").product._h, i64(n), i64(1), g, r, t, zz, work, state) != 0
    assert "another solver" in err()
    assert f(sol._h, prod._h, i64(n + 1), i64(1), g, r, t, zz, work, state) != 0 and "order" in err()
    assert f(sol._h, prod._h, i64(n), i64(0), g, r, t, zz, work, state) != 0 and "q" in err()
    assert f(sol._h, prod._h, i64(n), i64(1), g, r, t, zz, z, state) != 0 and "workspace pointer is NULL" in err()
    assert f(sol._h, prod._h, i64(n), i64(1), g, r, t, zz, P(24), state) != 0 and "16-byte aligned" in err()
    assert f(sol._h, prod._h, i64(n), i64(1), g, r, t, zz, work, z) != 0 and "state pointer is NULL" in err()
    for k, what in enumerate(("preconditioner", "r", "t", "z")):
        args = [g, r, t, zz]
        args[k] = z
        assert f(sol._h, prod._h, i64(n), i64(1), *args, work, state) != 0
        assert "the %s pointer of batch member 0 is NULL" % what in err()
    # a written operand (t and z included) that overlaps any other
    for args in ((g, r, t, t), (g, r, r, zz), (g, t, t, zz), (zz, r, t, zz), (g, r, t, P(base + 2 * (1 << 16) + 8))):
        assert f(sol._h, prod._h, i64(n), i64(1), *args, work, state) != 0 and "aliases" in err(), args
    assert lib.bsp_fsai_apply_batched_f64(sol._h, prod._h, i64(n), i64(1), z, z, z, z, work, state,
                                             ctypes.c_int32(0)) != 0
    assert "batch is empty" in err()
    # the build of kind 3 takes the checks of the other kinds; kind 4 is still unknown
    assert lib.bsp_cg_precond_build_f64(sol._h, prod._h, ctypes.c_int32(3), g, g, work, state) != 0 and "aliases" in err()
    assert lib.bsp_cg_precond_build_f64(sol._h, prod._h, ctypes.c_int32(4), g, r, work, state) != 0 and "kind" in err()
    with pytest.raises(ValueError, match="unknown built-in"):
        CG.Preconditioner(prod, "ilu", None)
