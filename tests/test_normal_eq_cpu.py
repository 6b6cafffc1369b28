"""CPU: the host maps of the normal equations of a sparse Jacobian.  The pair
table (offsets, order) and the figures of the map equal the numpy restatement on every case, the
device-byte formulas hold, bad input is refused by name, and JacobianPattern derives the structure that
SymmetricPattern derives from the expanded J^T J entries."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import sparse as S
import normal_eq_ref as R


@pytest.mark.parametrize("case", R.CASES)
def test_pair_table_and_info_match_the_restatement(case):
    c, pat = R.pattern(case)
    table, _ = R.reference(case)
    ka, kb, off = pat.normal_eq.pairTable()
    assert ka.dtype == np.int32 and kb.dtype == np.int32 and off.dtype == np.int64
    assert np.array_equal(ka, table[0]) and np.array_equal(kb, table[1]) and np.array_equal(off, table[2])
    assert np.all(c["cols"][ka] >= c["cols"][kb]) and np.all(c["rows"][ka] == c["rows"][kb])
    deg = np.bincount(c["rows"], minlength=c["m"])
    assert len(ka) == int((deg * (deg + 1) // 2).sum())
    assert pat.normal_eq.info() == R.ref_info(pat.solver, table, c["rows"], c["cols"], c["m"])


def test_cases_take_every_path():
    info = {name: R.pattern(name)[1].normal_eq.info() for name in R.CASES}
    assert info["hub"]["max_run"] in (301, 302) and info["hub"]["long_runs"] >= 4  # (0, 0) and (1..3, 0)
    deg = np.bincount(R.build("hub")["rows"])
    assert deg.max() == 70  # 2485 pairs in one row, 71 adjoint terms per entry: the wave path of the adjoint
    assert info["longrun"]["max_run"] == 12345 + 1
    assert info["empty"]["pairs"] == 0 and info["empty"]["destinations"] == 0
    assert info["one"]["pairs"] == 1 and info["one"]["tiles"] == 1
    assert info["tiles3"]["tiles"] == 3
    off = R.reference("tiles3")[0][2]
    runs_off, runs = np.unique(off, return_counts=True)
    assert sorted(set((runs_off[runs > R.LONG_RUN] // R.TILE).tolist())) == [0, 1, 2]
    assert len(R.pattern("blocks_elim")[1].solver.sparseEliminationRanges()) >= 2
    assert R.pattern("blocks")[1].solver.dataSize() > R.TILE  # more than one workgroup


def test_diag_offsets():
    for case in ("blocks", "blocks_elim", "tiles3"):
        sol = R.pattern(case)[1].solver
        d = sol.diagOffsets()
        assert d.dtype == np.int64 and d.shape == (sol.order(),)
        data = np.zeros(sol.dataSize())
        assert np.array_equal(np.sort(d), np.flatnonzero(sol.damp(data, 0.0, 1.0)))
        dense = np.zeros(sol.dataSize())
        dense[d] = 1 + np.arange(sol.order())
        assert np.array_equal(np.diag(sol.densify(dense)), 1 + np.arange(sol.order()))


def test_refusals():
    c, pat = R.pattern("scalar")
    sol, rows, cols, m, n = pat.solver, c["rows"], c["cols"], c["m"], c["n"]
    for bad_r, bad_c, text in ((m, 0, "is out of range"), (-1, 0, "is out of range"), (0, n, "is out of range"),
                               (0, -1, "is out of range")):
        r2, c2 = rows.copy(), cols.copy()
        r2[7], c2[7] = bad_r, bad_c
        with pytest.raises(RuntimeError, match=r"entry 7 at \(%d, %d\) %s" % (bad_r, bad_c, text)):
            sol.normalEquations(r2, c2, m)
    # entries 11 and 40 repeat the position of entry 5, entry 30 that of entry 2: 11 is the first repeat
    r2, c2 = rows.copy(), cols.copy()
    for k, k0 in ((40, 5), (11, 5), (30, 2)):
        r2[k], c2[k] = r2[k0], c2[k0]
    with pytest.raises(RuntimeError, match=r"entry 11 at \(%d, %d\) repeats the position of entry 5" % (r2[5], c2[5])):
        sol.normalEquations(r2, c2, m)
    # a row that couples two scalars of a solver whose pattern is diagonal
    diag = B.create_solver(B.Settings(), np.ones(4, dtype=np.int64), B.SparseStructure(np.arange(5), np.arange(4)))
    with pytest.raises(RuntimeError, match=r"entry 0 at \(0, 1\) and entry 1 .* columns \(3, 1\).*not in the solver's "
                                           "stored pattern"):
        diag.normalEquations([0, 0], [1, 3], 1)
    with pytest.raises(ValueError):
        sol.normalEquations(rows[:-1], cols, m)
    with pytest.raises(TypeError):
        sol.normalEquations(rows.astype(np.float64), cols, m)


def test_pair_count_limit_is_checked_before_allocating():
    """one Jacobian row of 65536 entries: P = 65536 * 65537 / 2 = 2^31 + 32768.  The solver is one dense
    param of 65536 scalars, built on the host only; the map must refuse from the row degrees alone"""
    n = 65536
    sol = B.create_solver(B.Settings(), np.array([n]), B.SparseStructure(np.array([0, 1]), np.array([0])))
    with pytest.raises(RuntimeError, match=r"P = %d pairs" % (n * (n + 1) // 2)):
        sol.normalEquations(np.zeros(n, dtype=np.int64), np.arange(n), 1)


def _expanded(c):
    """(rows, cols) of the lower entries of J^T J: every pair of every Jacobian row"""
    r, q = [], []
    for ks in R.row_groups(c["rows"], c["m"]):
        cs = c["cols"][ks]
        a, b = np.meshgrid(cs, cs, indexing="ij")
        r.append(np.maximum(a, b).ravel())
        q.append(np.minimum(a, b).ravel())
    return np.concatenate(r), np.concatenate(q)


@pytest.mark.parametrize("case", ["scalar", "blocks", "blocks_keep", "blocks_elim", "hub"])
def test_jacobian_pattern_structure(case):
    c, pat = R.pattern(case)
    er, ec = _expanded(c)
    sym = S.SymmetricPattern(er, ec, c["n"], param_sizes=c["param_sizes"], keep=c["keep"])
    assert np.array_equal(pat.structure.ptrs, sym.structure.ptrs)
    assert np.array_equal(pat.structure.inds, sym.structure.inds)
    assert np.array_equal(pat.solver.paramToSpan(), sym.solver.paramToSpan())
    assert pat.solver.dataSize() == sym.solver.dataSize() and pat.keep_span == sym.keep_span
    assert (pat.m, pat.n, pat.nnz) == (c["m"], c["n"], len(c["rows"]))
    if c["keep"] is not None:
        bar = int(pat.solver.skel()["spanStart"][pat.keep_span])
        internal = pat.solver.scalarPermutation()
        assert np.all(internal[c["keep"]] >= bar)
        assert np.all(np.delete(internal, c["keep"]) < bar)
        assert np.array_equal(pat._keep_dest, sym._keep_dest)


def test_map_of_another_solver_is_refused_on_the_host():
    """the check sits in front of any device work, so it can be seen without a device"""
    import ctypes
    c, pat = R.pattern("scalar")
    other = S.JacobianPattern(c["rows"], c["cols"], c["m"], c["n"]).solver
    lib, P = pat.solver._lib, ctypes.c_void_p
    buf = np.zeros(max(pat.solver.dataSize(), len(c["rows"])))
    rc = lib.bsp_normal_eq_hessian_f64(other._h, pat.normal_eq._h, P(buf.ctypes.data), P(buf.ctypes.data))
    assert rc != 0 and "another solver" in lib.bsp_last_error().decode()
